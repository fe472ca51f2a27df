"""Golden fixtures of tests/golden/ (test infrastructure).

A fixture NAME is one .npz archive, NAME.npz, or -- where one archive would pass the 1 MiB limit for a committed file -- a set of
archives NAME.part0.npz, NAME.part1.npz, ... whose keys are disjoint.  `load` reads either form as one archive; `save` writes the
second form whenever the first would be too large (the generators in tests/golden/ use it)."""
import io
import os
import re

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_FILE_BYTES = 1 << 20


class Archive:
    """The keys of every part of one fixture: `files` (in the order they were saved) and `archive[key]`."""

    def __init__(self, paths):
        self._parts = [np.load(p) for p in paths]
        self._part_of = {k: z for z in self._parts for k in z.files}
        self.files = [k for z in self._parts for k in z.files]

    def __getitem__(self, key):
        return self._part_of[key][key]

    def __contains__(self, key):
        return key in self._part_of


def part_paths(name, d=DIR):
    pat = re.compile(re.escape(name) + r"\.part(\d+)\.npz$")
    parts = sorted((int(m.group(1)), f) for f in os.listdir(d) for m in [pat.match(f)] if m)
    return [os.path.join(d, f) for _, f in parts] or [os.path.join(d, name + ".npz")]


def load(name, d=DIR):
    return Archive(part_paths(name, d))


def _npz_bytes(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def save(name, arrays, d=DIR, limit=MAX_FILE_BYTES):
    """Write `arrays` ({key: array}) as d/NAME.npz, or split in key order into parts of at most `limit` bytes each."""
    for f in os.listdir(d):
        if re.match(re.escape(name) + r"(\.part\d+)?\.npz$", f):
            os.remove(os.path.join(d, f))
    whole = _npz_bytes(arrays)
    if len(whole) <= limit:
        blobs = {name + ".npz": whole}
    else:
        blobs, cur, cur_bytes = {}, {}, b""
        for k, v in arrays.items():
            trial = _npz_bytes({**cur, k: v})
            if len(trial) > limit and cur:
                blobs["%s.part%d.npz" % (name, len(blobs))] = cur_bytes
                cur, trial = {}, _npz_bytes({k: v})
            if len(trial) > limit:
                raise ValueError("%s: array %r alone is %d bytes compressed (limit %d)" % (name, k, len(trial), limit))
            cur[k], cur_bytes = v, trial
        blobs["%s.part%d.npz" % (name, len(blobs))] = cur_bytes
    for f, blob in blobs.items():
        with open(os.path.join(d, f), "wb") as fh:
            fh.write(blob)
    return sorted(blobs)
