"""Host side of env snapshots (no GPU): the C ABI's error paths and the portable file format of EnvSnapshot."""
import ctypes as C

import numpy as np
import pytest

from conftest import synthetic_tables
from paintrl_amd import _lib
from paintrl_amd.device_tables import DeviceTables
from paintrl_amd.snapshot import FORMAT_VERSION, STATE_FIELDS, EnvSnapshot, decode_state, encode_state


def test_snapshot_symbols_reject_null_arguments():
    lib = _lib.load()
    assert hasattr(lib, 'prl_batch_export') and hasattr(lib, 'prl_batch_import')
    buf = C.c_void_p(0x1000)
    assert lib.prl_batch_export(None, 4, None, buf, buf, buf, None, buf, None) == -1
    assert b'null batch' in lib.prl_last_error()
    assert lib.prl_batch_import(None, 4, 4, None, None, buf, buf, buf, None, buf, None, None) == -1
    assert b'prl_batch_import' in lib.prl_last_error()
    assert lib.prl_batch_export(None, 4, None, None, None, None, None, None, None) == -1
    assert lib.prl_last_error()


def _synthetic(n, widths, rng, hsi=False):
    width = max(widths)
    words = (width + 63) // 64
    part = rng.randint(0, len(widths), size=n).astype(np.int32)
    painted = rng.randint(0, 2 ** 63, size=(n, words), dtype=np.int64).view(np.uint64)
    last = painted & rng.randint(0, 2 ** 63, size=(n, words), dtype=np.int64).view(np.uint64)
    for i in range(n):                                     # no bits past the row's own part
        bits = np.unpackbits(painted[i:i + 1].view(np.uint8), bitorder='little')
        bits[widths[part[i]]:] = 0
        painted[i] = np.packbits(bits, bitorder='little').view(np.uint64)
        last[i] &= painted[i]
    rec = rng.randn(n, 16)
    rec.view(np.int32)[:, 20:26] = rng.randint(-5, 1000, size=(n, 6))
    rec.view(np.int32)[:, 30:32] = rng.randint(0, 1000, size=(n, 2))
    rec.view(np.int32)[:, 24] = rng.randint(-2 ** 31, 2 ** 31 - 1, size=n)     # the episode counter: all 32 bits
    thick = rng.randint(0, 256, size=(n, width)).astype(np.uint8) if hsi else None
    return part, decode_state(rec), rec, painted, last, thick


@pytest.mark.parametrize('hsi', [False, True])
def test_canonical_file_round_trips(tmp_path, hsi):
    rng = np.random.RandomState(3)
    widths = [9664, 200]
    part, state, rec, painted, last, thick = _synthetic(7, widths, rng, hsi)
    snap = EnvSnapshot.from_canonical(part, ['a' * 64, 'b' * 64], widths, 'HSI' if hsi else 'RGB', state, painted, last, thick)
    path = str(tmp_path / 'snap.npz')
    snap.save(path)
    back = EnvSnapshot.load(path)
    assert len(back) == 7 and back.color_mode == snap.color_mode and back.fingerprints == snap.fingerprints
    assert back.n_samples == widths and np.array_equal(back.part, part)
    c = back.canonical()
    assert np.array_equal(c['painted'], painted) and np.array_equal(c['last'], last)
    assert (c['thick'] is None) == (not hsi) and (not hsi or np.array_equal(c['thick'], thick))
    assert np.array_equal(encode_state(c['state']).view(np.uint64), rec.view(np.uint64))     # the whole record, bit for bit
    z = np.load(path)
    assert int(z['format_version']) == FORMAT_VERSION
    assert {'state/' + f[0] for f in STATE_FIELDS} <= set(z.files)


def test_unknown_format_version_raises(tmp_path):
    rng = np.random.RandomState(4)
    part, state, _, painted, last, _ = _synthetic(2, [300], rng)
    path = str(tmp_path / 'snap.npz')
    EnvSnapshot.from_canonical(part, ['a' * 64], [300], 'RGB', state, painted, last).save(path)
    z = dict(np.load(path))
    z['format_version'] = np.int64(FORMAT_VERSION + 1)
    bad = str(tmp_path / 'bad.npz')
    np.savez(bad, **z)
    with pytest.raises(_lib.PaintRLError, match='format version'):
        EnvSnapshot.load(bad)
    del z['format_version']
    np.savez(bad, **z)
    with pytest.raises(_lib.PaintRLError, match='format version'):
        EnvSnapshot.load(bad)


def test_restore_checks_fingerprint_and_color_mode():
    door, sheet = DeviceTables(synthetic_tables('door_test')), DeviceTables(synthetic_tables('square'))
    assert door.fingerprint() != sheet.fingerprint() and len(door.fingerprint()) == 64
    assert DeviceTables(synthetic_tables('door_test')).fingerprint() == door.fingerprint()     # the samples, not the object
    rng = np.random.RandomState(5)
    part, state, _, painted, last, thick = _synthetic(3, [door.n_samples], rng, hsi=True)
    part[:] = 0
    snap = EnvSnapshot.from_canonical(part, [door.fingerprint()], [door.n_samples], 'HSI', state, painted, last, thick)
    assert list(snap.part_map([sheet, door], 'HSI')) == [1]
    with pytest.raises(_lib.PaintRLError, match='not a part of this batch'):
        snap.part_map([sheet], 'HSI')
    with pytest.raises(_lib.PaintRLError, match='COLOR_MODE'):
        snap.part_map([door], 'RGB')
    assert list(snap.part_map([sheet], 'HSI', rows=[])) == [-1]                # rows that are not restored are not checked
