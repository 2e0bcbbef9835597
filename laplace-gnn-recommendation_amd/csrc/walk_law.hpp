// The item -> user -> item walk law of the PinSAGE samplers (csrc/pinsage.hip) and of the random-walk matcher
// (csrc/walk_match.hip): the Philox counter layout of a draw and one traversal.  oracle/pinsage_ref.py (_words, _hop) restates
// both; every purpose number is named where it is used (11-16: pinsage.hip, 17: walk_match.hip).
#pragma once
#include "common.hpp"

namespace {

__device__ __forceinline__ MiPhilox pw(uint32_t purpose, uint32_t a, uint32_t b, uint32_t c, uint64_t seed, uint64_t step) {
    const uint32_t c3 = (purpose & 0xFFu) | ((uint32_t)(step & 0xFFFFFFu) << 8);
    return mi_philox4x32(a, b, c, c3, (uint32_t)seed, (uint32_t)((seed >> 32) ^ (step >> 24)));
}

struct Bip {
    const int32_t* iu_ptr; const int32_t* iu_idx;  // item -> users
    const int32_t* ui_ptr; const int32_t* ui_idx;  // user -> items
};

__device__ __forceinline__ int32_t hop(const Bip& g, int32_t item, uint32_t w0, uint32_t w1) {
    const int32_t b = g.iu_ptr[item], du = g.iu_ptr[item + 1] - b;
    if (du == 0) return -1;
    const int32_t u = g.iu_idx[b + (int32_t)(w0 % (uint32_t)du)];
    const int32_t b2 = g.ui_ptr[u], di = g.ui_ptr[u + 1] - b2;
    if (di == 0) return -1;
    return g.ui_idx[b2 + (int32_t)(w1 % (uint32_t)di)];
}

}  // namespace
