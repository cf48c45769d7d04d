"""EnvSnapshot: the state of some envs of a BatchedPaintEnv, to restore, clone or save (include/paintrl.h prl_batch_export).

What carries an env from one step to the next is its state record (16 doubles), its coverage row, its last-shot row and, for
COLOR_MODE 'HSI', its thickness row.  A snapshot taken from a batch holds these as device tensors in device sample order
(``BatchedPaintEnv.snapshot``); ``save`` writes them to a portable ``.npz`` in CANONICAL sample order (PartTables.sample_pix
order, ``DeviceTables.perm`` / ``inv_perm``), with the state record decoded to named fields, so that a file restores into a
batch of any size, on another GPU or in another process.  Each row names its part by index into ``fingerprints``
(``DeviceTables.fingerprint``: SHA-256 of the canonical sample positions, their count and the paint radius); a restore maps
them onto the target batch's parts and refuses parts it does not have and another color mode.
"""
import json

import numpy as np

from . import _lib

FORMAT_VERSION = 1

# the state record (include/paintrl.h prl_batch_get_state) as named fields: name -> (kind, index, width); kind 'f' indexes
# the 16 doubles, 'i' the 32 int32 words of the same record
STATE_FIELDS = [('pose', 'f', 0, 3), ('quat', 'f', 3, 4), ('last_turning_angle', 'f', 7, 1), ('total_reward', 'f', 8, 1),
                ('total_return', 'f', 9, 1), ('terminate', 'i', 20, 1), ('terminate_counter', 'i', 21, 1),
                ('last_on_part', 'i', 22, 1), ('step_counter', 'i', 23, 1), ('episode', 'i', 24, 1), ('facet_hint', 'i', 25, 1),
                ('last_episode_return', 'f', 13, 1), ('last_episode_reward', 'f', 14, 1), ('last_episode_len', 'i', 30, 1),
                ('last_episode_painted', 'i', 31, 1)]


def decode_state(raw):
    """float64 (N, 16) state records -> dict of named numpy arrays (``episode`` as uint64, the other ints as int32)."""
    r = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1, _lib.STATE_DOUBLES)
    ints = r.view(np.int32).reshape(r.shape[0], -1)
    out = {}
    for name, kind, i, w in STATE_FIELDS:
        src = r if kind == 'f' else ints
        v = src[:, i:i + w].copy() if w > 1 else src[:, i].copy()
        if name == 'episode':
            v = v.view(np.uint32).astype(np.uint64)
        out[name] = v
    return out


def encode_state(fields):
    """The inverse of ``decode_state``: dict of named arrays -> float64 (N, 16) state records."""
    n = np.asarray(fields['pose']).reshape(-1, 3).shape[0]
    r = np.zeros((n, _lib.STATE_DOUBLES), dtype=np.float64)
    ints = r.view(np.int32)
    for name, kind, i, w in STATE_FIELDS:
        v = np.asarray(fields[name])
        if kind == 'f':
            r[:, i:i + w] = v.reshape(n, w)
        elif name == 'episode':
            ints[:, i] = v.reshape(n).astype(np.uint64).astype(np.uint32).view(np.int32)
        else:
            ints[:, i] = v.reshape(n).astype(np.int32)
    return r


def _pack_bits(bits):
    """bool (N, P) -> uint64 (N, ceil(P / 64)), bit s & 63 of word s >> 6 = sample s."""
    n, p = bits.shape
    words = (p + 63) // 64
    b = np.packbits(bits, axis=1, bitorder='little')
    out = np.zeros((n, words * 8), dtype=np.uint8)
    out[:, :b.shape[1]] = b
    return out.view(np.uint64)


def _unpack_bits(words, p):
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return np.unpackbits(w.view(np.uint8), axis=-1, bitorder='little')[..., :p].astype(bool)


class EnvSnapshot(object):
    """State of ``len(snapshot)`` envs.  ``part`` (int32 per row) indexes ``fingerprints`` / ``n_samples``; ``color_mode`` is
    'RGB' or 'HSI'.  A snapshot of a batch holds device tensors (``state`` float64 (n, 16), ``painted`` / ``last`` int64
    (n, mask_stride), ``thick`` uint8 (n, 64 * mask_stride) or None, in device sample order of ``tables``); one loaded from a
    file holds the canonical arrays only.  ``canonical()`` gives the portable form of either."""

    def __init__(self, part, fingerprints, n_samples, color_mode, device_rows=None, tables=None, mask_stride=None,
                 canonical=None):
        self.part = np.ascontiguousarray(part, dtype=np.int32).reshape(-1)
        self.fingerprints = [str(f) for f in fingerprints]
        self.n_samples = [int(p) for p in n_samples]
        if color_mode not in ('RGB', 'HSI'):
            raise _lib.PaintRLError('color mode %r is neither RGB nor HSI' % (color_mode,))
        self.color_mode = color_mode
        self.mask_stride = mask_stride
        self.tables = tables
        if device_rows is not None:
            self.state, self.painted, self.last, self.thick, self.part_dev = device_rows
        else:
            self.state = self.painted = self.last = self.thick = self.part_dev = None
        self._canon = canonical

    def __len__(self):
        return int(self.part.shape[0])

    # ------------------------------------------------------------------ canonical form
    @classmethod
    def from_canonical(cls, part, fingerprints, n_samples, color_mode, state, painted, last, thick=None):
        """A snapshot from canonical arrays: ``state`` a dict of STATE_FIELDS, ``painted`` / ``last`` uint64
        (n, ceil(max(n_samples) / 64)) words in canonical sample order, ``thick`` uint8 (n, max(n_samples)) for 'HSI'."""
        n = np.asarray(part).reshape(-1).shape[0]
        width = max(int(p) for p in n_samples)
        words = (width + 63) // 64
        canon = {'state': {name: np.asarray(state[name]) for name, _, _, _ in STATE_FIELDS},
                 'painted': np.ascontiguousarray(painted, dtype=np.uint64).reshape(n, words),
                 'last': np.ascontiguousarray(last, dtype=np.uint64).reshape(n, words),
                 'thick': None if thick is None else np.ascontiguousarray(thick, dtype=np.uint8).reshape(n, width)}
        if (canon['thick'] is not None) != (color_mode == 'HSI'):
            raise _lib.PaintRLError('thickness bytes are required exactly for COLOR_MODE HSI')
        return cls(part, fingerprints, n_samples, color_mode, canonical=canon)

    def canonical(self):
        """dict(state=named fields, painted, last=uint64 (n, words), thick=uint8 (n, width) or None), canonical sample order;
        rows of a mixed snapshot are padded to the widest part (zero bits, thickness 255)."""
        if self._canon is not None:
            return self._canon
        n, width = len(self), max(self.n_samples)
        words = (width + 63) // 64
        state = decode_state(self.state.cpu().numpy())
        painted_dev = self.painted.cpu().numpy().view(np.uint64)
        last_dev = self.last.cpu().numpy().view(np.uint64)
        thick_dev = None if self.thick is None else self.thick.cpu().numpy()
        painted = np.zeros((n, words), dtype=np.uint64)
        last = np.zeros((n, words), dtype=np.uint64)
        thick = None if thick_dev is None else np.full((n, width), 255, dtype=np.uint8)
        for p in np.unique(self.part):
            rows = np.nonzero(self.part == p)[0]
            t = self.tables[p]
            for src, dst in ((painted_dev, painted), (last_dev, last)):
                bits = np.zeros((rows.size, width), dtype=bool)
                bits[:, :t.n_samples] = t.mask_to_canonical(src[rows])
                dst[rows] = _pack_bits(bits)
            if thick is not None:
                thick[rows, :t.n_samples] = thick_dev[rows][:, t.inv_perm]
        self._canon = {'state': state, 'painted': painted, 'last': last, 'thick': thick}
        return self._canon

    def save(self, path):
        """Write the portable ``.npz`` (canonical sample order, named state fields, format version, fingerprints)."""
        c = self.canonical()
        arrays = {'format_version': np.int64(FORMAT_VERSION), 'part': self.part,
                  'fingerprints': np.array(json.dumps(self.fingerprints)), 'n_samples': np.asarray(self.n_samples, np.int64),
                  'color_mode': np.array(self.color_mode), 'painted': c['painted'], 'last': c['last']}
        if c['thick'] is not None:
            arrays['thick'] = c['thick']
        for name, _, _, _ in STATE_FIELDS:
            arrays['state/' + name] = np.asarray(c['state'][name])
        with open(path, 'wb') as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path):
        z = np.load(path, allow_pickle=False)
        version = int(z['format_version']) if 'format_version' in z.files else None
        if version != FORMAT_VERSION:
            raise _lib.PaintRLError('%s: snapshot format version %r, this library reads %d' % (path, version, FORMAT_VERSION))
        state = {name: z['state/' + name] for name, _, _, _ in STATE_FIELDS}
        return cls.from_canonical(z['part'], json.loads(str(z['fingerprints'])), z['n_samples'], str(z['color_mode']),
                                  state, z['painted'], z['last'], z['thick'] if 'thick' in z.files else None)

    # ------------------------------------------------------------------ restoring
    def part_map(self, parts, color_mode, rows=None):
        """Part index of the snapshot -> part index among ``parts`` (DeviceTables) with the same fingerprint, int32 (-1 = the
        part is not there).  Raises PaintRLError on another color mode, or if a part that ``rows`` (default: all rows) use has
        no counterpart."""
        if color_mode != self.color_mode:
            raise _lib.PaintRLError('the snapshot has COLOR_MODE %s, the batch %s' % (self.color_mode, color_mode))
        have = [p.fingerprint() for p in parts]
        m = np.array([have.index(f) if f in have else -1 for f in self.fingerprints], dtype=np.int32)
        used = np.unique(self.part if rows is None else self.part[np.asarray(rows, dtype=np.int64)])
        for p in used:
            if p < 0 or p >= m.size or m[p] < 0:
                raise _lib.PaintRLError('snapshot part %d (fingerprint %s) is not a part of this batch'
                                        % (p, self.fingerprints[p] if 0 <= p < m.size else '?'))
        return m

    def device_rows(self, batch, part_map):
        """(state, painted, last, thick, part) device tensors in ``batch``'s layout, part ids of the batch."""
        torch = __import__('torch')
        dev = batch.device
        known = (self.part >= 0) & (self.part < part_map.size)
        part = torch.as_tensor(np.where(known, part_map[np.where(known, self.part, 0)], -1), dtype=torch.int32, device=dev)
        if self.state is not None and self.mask_stride == batch.mask_stride and self.state.device == dev and \
                all(self.tables[p] is batch.parts[part_map[p]] or np.array_equal(self.tables[p].perm, batch.parts[part_map[p]].perm)
                    for p in np.unique(self.part) if 0 <= p < part_map.size and part_map[p] >= 0):
            return self.state, self.painted, self.last, self.thick, part
        c = self.canonical()
        n, ms = len(self), batch.mask_stride
        painted = np.zeros((n, ms), dtype=np.uint64)
        last = np.zeros((n, ms), dtype=np.uint64)
        thick = None if c['thick'] is None else np.full((n, 64 * ms), 255, dtype=np.uint8)
        for p in np.unique(self.part):
            if not (0 <= p < part_map.size) or part_map[p] < 0:
                continue                                     # (rows the caller does not restore)
            rows = np.nonzero(self.part == p)[0]
            t = batch.parts[part_map[p]]
            for src, dst in ((c['painted'], painted), (c['last'], last)):
                bits = np.zeros((rows.size, 64 * ms), dtype=bool)
                bits[:, t.inv_perm] = _unpack_bits(src[rows], t.n_samples)
                dst[rows] = _pack_bits(bits)
            if thick is not None:
                thick[rows[:, None], t.inv_perm[None, :]] = c['thick'][rows, :t.n_samples]
        as_dev = lambda a: torch.from_numpy(a).to(dev)                                  # noqa: E731
        return (as_dev(encode_state(c['state'])), as_dev(painted.view(np.int64)), as_dev(last.view(np.int64)),
                None if thick is None else as_dev(thick), part)
