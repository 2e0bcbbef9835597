"""A/B of the sliced short-row launch (ops.ROW_SLICES, mi_spmm_ex.row_slices) on the bench workload, in ONE process:
    python3 tools/ab_row_slices.py [--config c4|c2] [--settings 0,2,4,2:1] [--steps 20] [--warmup 5]
One generated graph and one trainer; per setting bench.timed_steps (the trainer goes on training across settings, so
the losses differ; bench.py --dump-outputs compares results).  Prints ms per step (mean, p10 / p50 / p90) and the average
dense / dense + Adam epilogue / sparse-operand launch."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as t
import bench
from laplace_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument('--config', default='c4')
ap.add_argument('--settings', default='0,2,4,0,2,4')
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=5)
a = ap.parse_args()
args = argparse.Namespace(config=a.config, users=None, items=None, edges=None, dim=128, layers=3, batch=None, uniform=False,
                          no_reorder=False)
w = bench.build_workload(a.config, args, 1, 0, t.device('cuda:0'))
trainer = w['trainer']
for setting in a.settings.split(','):   # S or S:F (F = ops.ROW_SLICES_FORMS: bit 0 dense, 1 Adam epilogue, 2 x_map)
    s, _, f = setting.partition(':')
    s, ops.ROW_SLICES_FORMS = int(s), int(f or 7)
    ops.ROW_SLICES = s
    elapsed, per, events, loss = bench.timed_steps(trainer, a.steps, a.warmup, t.cuda.synchronize)
    kinds = {}
    for e0, e1, kind, _, _, _ in events:
        kinds.setdefault(kind, []).append(e0.elapsed_time(e1))
    avg = '  '.join(f'{k} {sum(v) / len(v):.3f}' for k, v in sorted(kinds.items()))
    n = len(per)
    print(f'row_slices {setting}: ms/step {1e3 * elapsed / a.steps:.3f} (p10 {per[n // 10]:.2f} p50 {per[n // 2]:.2f} p90 {per[(9 * n) // 10]:.2f})  '
          f'launch ms: {avg}  loss {float(loss):.8f}', flush=True)
