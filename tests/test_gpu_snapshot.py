"""GPU: env snapshots -- export / import kernels, BatchedPaintEnv.snapshot / restore / copy_envs, the portable file format,
and PaintGymEnv.get_state / set_state.  "Equal" is bit for bit: every obs, final_obs, reward, done and info row, the painted,
last-shot and thickness words and the whole state record."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_episodes, synthetic_tables

pytestmark = pytest.mark.gpu

BIG = ('door_rr_big', (652, 652))            # 70 411 samples: the class of the reference's door_rr_big (70 654)
MID = ('door_rr_big', (320, 320))            # 17 k samples: the smallest large part


def _tables(spec):
    name, tex = spec if isinstance(spec, tuple) else (spec, None)
    return synthetic_tables(name, tex_size=tex)


def _env(parts, n, env_part_id=None, **kw):
    from paintrl_amd.batched_env import BatchedPaintEnv
    from paintrl_amd.device_tables import DeviceTables
    dts = [DeviceTables(_tables(p)) for p in parts]
    return BatchedPaintEnv(dts, n, env_part_id=env_part_id, device='cuda:0', **kw)


def _dump(env):
    """Everything that carries over from one step to the next, as host arrays (device order)."""
    import torch
    from paintrl_amd import _lib
    out = {'painted': env.painted_words().cpu().numpy(), 'last': env.last_shot_words()[0].cpu().numpy()}
    rec = torch.zeros((env.n_envs, 16), dtype=torch.float64, device=env.device)
    env.state_into(rec)
    out['state'] = rec.cpu().numpy().view(np.uint64)
    if env.cfg.color_mode == 1:
        raw = torch.zeros((env.n_envs, 64 * env.mask_stride), dtype=torch.uint8, device=env.device)
        _lib.check(env.lib.prl_batch_get_thickness(env._batch, C.c_void_p(raw.data_ptr()), env._stream()), 'thickness')
        out['thick'] = raw.cpu().numpy()
    return out


def _run(env, actions, starts=None):
    """Step through ``actions`` (T, N); every output row of every step, then the final dump."""
    rows = []
    for t in range(actions.shape[0]):
        o, r, d, i = env.step(actions[t], start_idx=None if starts is None else starts[t])
        done = d.cpu().numpy().copy()
        final = env.final_obs.cpu().numpy().copy()
        final[~done] = 0                                  # (rows of envs that did not finish are not written by the step)
        rows.append((o.cpu().numpy().copy(), final, r.cpu().numpy().copy(), done, i.cpu().numpy().copy()))
    return rows, _dump(env)


def _same(a, b, sel_a=slice(None), sel_b=slice(None)):
    rows_a, dump_a = a
    rows_b, dump_b = b
    for t, (ra, rb) in enumerate(zip(rows_a, rows_b)):
        for k, (x, y) in enumerate(zip(ra, rb)):
            x, y = x[sel_a], y[sel_b]
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), 'step %d output %d differs' % (t, k)
    for key in dump_a:
        assert np.array_equal(dump_a[key][sel_a], dump_b[key][sel_b]), key + ' differs'


RESUME = {
    'door_section': (['door_test'], 4096, None, dict()),
    'door_grid_overlap': (['door_test'], 4096, None, dict(obs_mode='grid', overlap_penalty=True)),
    'door_atan2_sectors': (['door_test'], 4096, None, dict(obs_grad=6, overlap_penalty=True)),
    'door_hsi': (['door_test'], 1024, None, dict(color_mode='HSI', overlap_penalty=True)),
    'door_cone_beams': (['door_test'], 128, None, dict(paint_method='normal', overlap_penalty=True)),
    'big_70k': ([BIG], 512, None, dict(overlap_penalty=True)),
    'mixed_small_big': (['door_test', MID], 512, np.arange(512) % 2, dict(overlap_penalty=True, max_possible_point=[9148, 17000])),
}


@pytest.mark.parametrize('case', sorted(RESUME))
def test_resume_equals_uninterrupted(case):
    parts, n, ids, kw = RESUME[case]
    env = _env(parts, n, ids, auto_reset=True, seed=11, max_episode_len=12, **kw)
    rng = np.random.RandomState(1)
    env.reset()
    _run(env, rng.randint(0, 4, size=(5, n)))
    snap = env.snapshot()
    acts = rng.randint(0, 4, size=(20, n))
    a = _run(env, acts)
    assert sum(r[3].sum() for r in a[0]) > 0                      # episodes end (and auto-reset) inside the m steps
    obs = env.restore(snap)
    assert np.array_equal(obs.cpu().numpy(), env.observe().cpu().numpy())
    b = _run(env, acts)
    _same(a, b)
    env.close()


def test_resume_through_rollout_fragment():
    import torch
    n, k, m = 512, 4, 16
    env = _env(['door_test'], n, auto_reset=True, seed=5, max_episode_len=10, overlap_penalty=True)
    rng = np.random.RandomState(2)
    dev = env.device

    def fragment(acts):
        t = acts.shape[0]
        obs = torch.zeros((t + 1, n, env.obs_dim), dtype=torch.float64, device=dev)
        obs[0] = env.observe()
        out = dict(obs=obs, final_obs=torch.zeros((t, n, env.obs_dim), dtype=torch.float64, device=dev),
                   reward=torch.zeros((t, n), dtype=torch.float64, device=dev), done_u8=torch.zeros((t, n), dtype=torch.uint8, device=dev),
                   info=torch.zeros((t, n, 2), dtype=torch.float64, device=dev))
        env.rollout_fragment(t, action=torch.as_tensor(acts, dtype=torch.int32, device=dev).contiguous(), **out)
        return [v.cpu().numpy() for v in out.values()], _dump(env)

    env.reset()
    fragment(rng.randint(0, 4, size=(k, n)))
    snap = env.snapshot()
    acts = rng.randint(0, 4, size=(m, n))
    a = fragment(acts)
    assert a[0][3].sum() > 0
    env.restore(snap)
    b = fragment(acts)
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y)
    for key in a[1]:
        assert np.array_equal(a[1][key], b[1][key]), key
    env.close()


def test_into_fresh_batch_and_through_a_file(tmp_path):
    from paintrl_amd.snapshot import EnvSnapshot
    n, k, m = 256, 6, 14
    kw = dict(auto_reset=True, seed=3, max_episode_len=9, overlap_penalty=True, color_mode='HSI')
    a_env = _env(['door_test'], n, **kw)
    rng = np.random.RandomState(3)
    a_env.reset()
    _run(a_env, rng.randint(0, 4, size=(k, n)))
    snap = a_env.snapshot()
    subset = np.array([200, 3, 77, 150, 4])
    path = str(tmp_path / 'snap.npz')
    a_env.snapshot(subset).save(path)
    acts = rng.randint(0, 4, size=(m, n))
    starts = rng.randint(0, 4, size=(m, n))
    a = _run(a_env, acts, starts)
    # the same parts and seed, a new batch: the export lands there and continues as A did (library start-point draws too)
    b_env = _env(['door_test'], n, **kw)
    b_env.restore(snap)
    b = _run(b_env, acts, starts)
    _same(a, b)
    # a file, a batch of another size, a subset of rows, explicit start points
    c_env = _env(['door_test'], subset.size, **dict(kw, seed=99))
    c_env.reset()
    loaded = EnvSnapshot.load(path)
    c_env.restore(loaded)
    c = _run(c_env, acts[:, subset], starts[:, subset])
    _same(a, c, sel_a=subset)
    for e in (a_env, b_env, c_env):
        e.close()


@pytest.mark.parametrize('kw', [dict(overlap_penalty=True), dict(color_mode='HSI', overlap_penalty=True)])
def test_canonical_snapshot_of_the_oracle_continues_like_the_oracle(kw):
    import oracle
    from paintrl_amd.snapshot import EnvSnapshot
    tables = _tables('door_test')
    n, k, m = 64, 12, 12
    orc = oracle.Oracle(tables, n, **kw)
    rng = np.random.RandomState(4)
    start = rng.randint(0, orc.n_start, size=n)
    orc.reset(start)
    for _ in range(k):
        orc.step(rng.randint(0, 4, size=n))
    env = _env(['door_test'], n, **kw)
    e = orc.env
    state = {'pose': np.array([e[i].pose[:] for i in range(n)]), 'quat': np.array([e[i].quat[:] for i in range(n)]),
             'last_turning_angle': np.array([e[i].last_turning_angle for i in range(n)]),
             'total_reward': np.array([e[i].total_reward for i in range(n)]),
             'total_return': np.array([e[i].total_return for i in range(n)]),
             'terminate': np.array([e[i].terminate for i in range(n)]),
             'terminate_counter': np.array([e[i].terminate_counter for i in range(n)]),
             'last_on_part': np.array([e[i].last_on_part for i in range(n)]),
             'step_counter': np.array([e[i].step_counter for i in range(n)]),
             'episode': np.ones(n, dtype=np.uint64), 'facet_hint': -np.ones(n, dtype=np.int32),
             'last_episode_return': np.zeros(n), 'last_episode_reward': np.zeros(n),
             'last_episode_len': np.zeros(n, dtype=np.int32), 'last_episode_painted': np.zeros(n, dtype=np.int32)}
    hsi = kw.get('color_mode') == 'HSI'
    snap = EnvSnapshot.from_canonical(np.zeros(n, np.int32), [env.parts[0].fingerprint()], [env.parts[0].n_samples],
                                      'HSI' if hsi else 'RGB', state, orc.painted, orc.last, orc.thick if hsi else None)
    obs = env.restore(snap)
    assert np.array_equal(obs.cpu().numpy(), orc.observe())
    for t in range(m):
        acts = rng.randint(0, 4, size=n)
        o, r, d, i = env.step(acts)
        oo, rr, dd, ii = orc.step(acts)
        assert np.array_equal(o.cpu().numpy(), oo) and np.array_equal(d.cpu().numpy(), dd), 'step %d' % t
        if hsi:        # the oracle sums a shot's HSI deposits in sample order, the reference (and the GPU) in another: 1e-12
            assert np.allclose(r.cpu().numpy(), rr, rtol=0, atol=1e-12) and np.allclose(i.cpu().numpy(), ii, rtol=0, atol=1e-12)
        else:
            assert np.array_equal(r.cpu().numpy(), rr) and np.array_equal(i.cpu().numpy(), ii), 'step %d' % t
    for i in range(n):
        assert np.array_equal(env.painted_bits(i), orc.painted_bits(i))
    if hsi:
        assert np.array_equal(env.thickness(), orc.thick)
    env.close()


def test_clone_one_env_into_all():
    n, k, m = 512, 7, 20
    env = _env(['door_test'], n, auto_reset=True, seed=8, max_episode_len=11, overlap_penalty=True)
    rng = np.random.RandomState(6)
    env.reset()
    _run(env, rng.randint(0, 4, size=(k, n)))
    env.copy_envs(np.arange(n), np.zeros(n, dtype=np.int64))
    acts = np.repeat(rng.randint(0, 4, size=(m, 1)), n, axis=1)
    starts = np.repeat(rng.randint(0, 4, size=(m, 1)), n, axis=1)
    rows, dump = _run(env, acts, starts)
    assert sum(r[3][0] for r in rows) > 0
    for t, row in enumerate(rows):
        for x in row:
            assert (x == x[:1]).all(), 'step %d: a clone differs from env 0' % t
    for key, v in dump.items():
        assert (v == v[:1]).all(), key
    env.close()


@pytest.mark.parametrize('part', ['door_test', MID])
def test_swap_and_three_cycle_and_exact_last_index(part):
    import torch
    n = 64
    env = _env([part], n, auto_reset=True, seed=2, max_episode_len=30, overlap_penalty=True)
    rng = np.random.RandomState(7)
    env.reset()
    _run(env, rng.randint(0, 4, size=(6, n)))
    before = _dump(env)
    dst, src = [0, 1, 4, 5, 3], [1, 0, 3, 4, 5]
    env.copy_envs(dst, src)                                             # host indices
    after = _dump(env)
    perm = np.arange(n)
    perm[dst] = src
    for key in before:
        assert np.array_equal(after[key], before[key][perm]), key
    env.copy_envs(torch.tensor(src, dtype=torch.int32, device=env.device),      # device indices: back again
                  torch.tensor(dst, dtype=torch.int32, device=env.device))
    for key in before:
        assert np.array_equal(_dump(env)[key], before[key]), key
    # the imported last-shot index is exact: bit w & 63 of word w >> 6 set exactly for the non-zero words w
    env.restore(env.snapshot())
    last, nz = env.last_shot_words()
    last, nz = last.cpu().numpy(), nz.cpu().numpy().view(np.uint64)
    for e in range(n):
        want = np.zeros(nz.shape[1] * 64, dtype=bool)
        want[:last.shape[1]] = last[e] != 0
        assert np.array_equal(np.unpackbits(nz[e].view(np.uint8), bitorder='little').astype(bool), want), e
    assert (last != 0).any()
    env.close()


def test_bad_pairs_are_skipped_counted_and_raise():
    import torch
    from paintrl_amd import _lib
    n = 16
    env = _env(['door_test', 'square'], n, np.arange(n) % 2, auto_reset=True, seed=4, max_possible_point=[9148, 14350])
    rng = np.random.RandomState(8)
    env.reset()
    _run(env, rng.randint(0, 4, size=(5, n)))
    snap = env.snapshot()
    _run(env, rng.randint(0, 4, size=(5, n)))
    moved = _dump(env)
    with pytest.raises(_lib.PaintRLError, match='2 of 3'):
        env.restore(snap, envs=[0, 1, n + 5], rows=[1, 1, 0])            # 0 <- 1: another part; n + 5: out of range
    now = _dump(env)
    for key in now:
        assert np.array_equal(now[key][0], moved[key][0]), key              # untouched
        assert np.array_equal(now[key][2:], moved[key][2:]), key
    assert np.array_equal(now['state'][1], snap.state.cpu().numpy().view(np.uint64)[1])
    # the raw form: nothing checked on the host, the kernel counts
    cnt = torch.zeros(1, dtype=torch.int32, device=env.device)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=env.device)        # noqa: E731
    env.restore_raw(i32([2, -1, 3, 4]), i32([2, 0, n, 5]), snap.state, snap.painted, snap.last, None, snap.part_dev,
                    n=4, n_skipped=cnt)
    assert int(cnt.item()) == 3                                         # env -1; row n (out of range); 4 <- 5: parts differ
    assert np.array_equal(_dump(env)['painted'][3], now['painted'][3])
    env.close()


def test_gym_env_get_and_set_state_replays_the_golden_episode(tmp_path):
    from paintrl_amd import PaintGymEnv, synth_parts
    root = str(tmp_path / 'root')
    synth_parts.write_synthetic_parts(root)
    ep = load_episodes('sheet')['g2_zigzag']
    PaintGymEnv.change_action_mode(1, 'discrete', 4)
    PaintGymEnv.change_obs_mode('simple', 4)
    cfg = dict(PaintGymEnv.EXTRA_CONFIG, Part_NO=1, START_POINT_MODE='fixed')
    save_at = 50
    assert len(ep['actions']) > save_at + 10
    with PaintGymEnv(root, with_robot=False, rollout=True, extra_config=cfg) as env:
        env.reset()
        for a in ep['actions'][:save_at]:
            env.step(int(a))
        saved = env.get_state()

        def finish():
            out = []
            for k in range(save_at, len(ep['actions'])):
                obs, r, done, info = env.step(int(ep['actions'][k]))
                assert np.array_equal(obs, ep['obs'][k]) and r == ep['reward'][k] and done == bool(ep['done'][k]), k
                out.append((obs, r, done, info, env.robot.get_angle_diff(), env._step_counter))
            return out, env.get_job_status(), list(env.replay_buffer)

        first = finish()
        env.set_state(saved)
        second = finish()
        assert first[1] == second[1] == int(np.unpackbits(ep['snaps'][-1], bitorder='little').sum())
        assert len(first[0]) == len(second[0])
        for x, y in zip(first[0], second[0]):
            assert np.array_equal(x[0], y[0]) and x[1:] == y[1:]
        assert first[2] == second[2]
    PaintGymEnv.change_obs_mode('section', 4)
