"""Golden fixtures under tests/golden/: one <name>.npz each or, for a fixture that would exceed the size of a
committed file, the same arrays spread over <name>.part0.npz, <name>.part1.npz, ...  save() splits where
needed, load() joins the parts back into one mapping with the .files / [key] interface of np.load."""
import glob
import io
import os

import numpy as np

PART_BYTES = 900 * 1024          # compressed bytes per file (committed files stay below 1 MiB)


class Parts(dict):
    @property
    def files(self):
        return list(self)


def _parts(path):
    stem = path[:-len(".npz")]
    found = glob.glob(glob.escape(stem) + ".part*.npz")
    return sorted(found, key=lambda p: int(p[len(stem) + len(".part"):-len(".npz")]))


def load(path):
    if os.path.exists(path):
        return np.load(path)
    parts = _parts(path)
    if not parts:
        raise FileNotFoundError(path)
    out = Parts()
    for p in parts:
        with np.load(p) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _size(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.tell()


def save(path, **arrays):
    """np.savez_compressed(path, **arrays), split into <name>.partN.npz files of at most PART_BYTES when the whole
    would be larger (keys keep their order; one array is never split).  Returns the paths written."""
    for old in _parts(path) + ([path] if os.path.exists(path) else []):
        os.remove(old)
    if _size(arrays) <= PART_BYTES:
        np.savez_compressed(path, **arrays)
        return [path]
    groups, cur = [], {}
    for k, v in arrays.items():
        if cur and _size({**cur, k: v}) > PART_BYTES:
            groups.append(cur)
            cur = {}
        cur[k] = v
    groups.append(cur)
    written = []
    for i, g in enumerate(groups):
        p = f"{path[:-len('.npz')]}.part{i}.npz"
        np.savez_compressed(p, **g)
        assert os.path.getsize(p) < 1 << 20, (p, os.path.getsize(p))
        written.append(p)
    return written
