"""Timing of the snapshot kernels (prl_batch_export / prl_batch_import, BatchedPaintEnv.copy_envs) at 4 096 envs: the door
(RGB and HSI) and a 70 k-sample part (door_rr_big at texture 652, as tools/bench_big_parts.sh builds it).  HIP events around
back-to-back launches; run under `rocprofv3 --kernel-trace --stats` for the kernels' own durations.  Prints one JSON line per
case: microseconds per call, bytes moved (read + written) and the fraction of 6.3 TB/s (the achievable HBM rate) that is.
    python tools/snapshot_timing.py [--out FILE]"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from paintrl_amd import part_tables, synth_parts  # noqa: E402
from paintrl_amd.batched_env import BatchedPaintEnv  # noqa: E402
from paintrl_amd.device_tables import DeviceTables  # noqa: E402

HBM = 6.3e12            # bytes / s achievable (MI355X_MICROARCH.md)
N = 4096


def timed(fn, reps=50):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps          # us per call


def case(name, part, tex, **kw):
    tables = part_tables.build_part_tables(mesh=synth_parts.synthetic_mesh(part), tex_size=(tex, tex), name=part)
    env = BatchedPaintEnv(DeviceTables(tables), N, auto_reset=True, seed=1, max_possible_point=int(0.95 * tables.sample_pos.shape[0]),
                          **kw)
    env.reset()
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    for _ in range(20):                               # painted rows, last-shot rows with words set
        env.step_raw(torch.randint(0, 4, (N,), generator=gen, device='cuda', dtype=torch.int32))
    torch.cuda.synchronize()
    ms = env.mask_stride
    hsi = kw.get('color_mode') == 'HSI'
    row = 16 * 8 + 2 * ms * 8 + (64 * ms if hsi else 0)
    bufs = (torch.empty((N, 16), dtype=torch.float64, device='cuda'), torch.empty((N, ms), dtype=torch.int64, device='cuda'),
            torch.empty((N, ms), dtype=torch.int64, device='cuda'),
            torch.empty((N, 64 * ms), dtype=torch.uint8, device='cuda') if hsi else None,
            torch.empty(N, dtype=torch.int32, device='cuda'))
    perm = torch.randperm(N, generator=gen, device='cuda').to(torch.int32)
    src = perm.cpu().numpy()
    dst = np.roll(src, 1)                                 # a rotation of all envs: every row moves
    t_exp = timed(lambda: env.snapshot_into(perm, *bufs))
    t_imp = timed(lambda: env.restore_raw(perm, None, *bufs))
    t_copy = timed(lambda: env.copy_envs(torch.from_numpy(dst).cuda(), torch.from_numpy(src).cuda()))
    d_dev, s_dev = torch.from_numpy(dst).cuda(), torch.from_numpy(src).cuda()
    t_copy_dev = timed(lambda: env.copy_envs(d_dev, s_dev))
    one = 2 * N * row                                      # read + written by one export or one import
    out = dict(case=name, n_envs=N, n_samples=int(tables.sample_pos.shape[0]), mask_stride=ms, row_bytes=row,
               export_us=round(t_exp, 2), import_us=round(t_imp, 2), copy_envs_us=round(t_copy_dev, 2),
               copy_envs_with_index_upload_us=round(t_copy, 2), export_bytes=one, import_bytes=one, copy_envs_bytes=2 * one,
               export_frac_hbm=round(one / (t_exp * 1e-6) / HBM, 3), import_frac_hbm=round(one / (t_imp * 1e-6) / HBM, 3),
               copy_envs_frac_hbm=round(2 * one / (t_copy_dev * 1e-6) / HBM, 3))
    env.close()
    return out


def main():
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    lines = [case('door_rgb', 'door_test', 240), case('door_hsi', 'door_test', 240, color_mode='HSI'),
             case('door_rr_big_652', 'door_rr_big', 652)]
    text = '\n'.join(json.dumps(x) for x in lines)
    print(text, flush=True)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
