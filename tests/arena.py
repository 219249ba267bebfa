"""A fenced arena for one call under test: ONE byte allocation from which every buffer of the call is cut -- inputs,
workspace, outputs -- each between two guard bands, so that a store outside an output or outside the caller's workspace,
or a load past the end of an input, lands in memory that belongs to the test and shows.

Layout, from the arena's base:

    [front guard >= 64 KiB][body][behind guard >= 64 KiB, up to the next multiple of 256] ... [1 MiB of slack]

* every body starts at a multiple of 256 bytes from the base (what the device allocator gives; the base itself is
  asserted to be 256-aligned on the device); its behind guard starts at the very next byte, whatever the body's size;
* guards of INPUTS hold 0xFF bytes: NaN as float32 / float64, -1 as int32 / int64 -- a load past an input that reaches
  a result poisons it;  guards of WORKSPACE and OUTPUTS hold 0xA5;
* output bodies hold 0xFF, the workspace body a byte the caller chooses, input bodies the caller's values;
* the slack behind the last guard holds 0xA5 and is checked as the tail of the last region's behind guard.

The arena is assembled on the host as one byte image and uploaded once; `read()` brings all of it back, `check()`
compares the guards of what came back with the image and names every guard of which any byte changed.  `reset()` puts
the image back (with another workspace fill if asked), so a call can be repeated on the same addresses.

The helper knows nothing of the library: it hands out addresses and compares bytes.  backend "numpy" keeps the arena in
a NumPy byte array through the same code (tests/test_arena_host.py plants writes into it); backend "torch" keeps it in
one torch.uint8 tensor on the current device.
"""
import numpy as np

ALIGN = 256
GUARD = 64 * 1024
SLACK = 1024 * 1024
INPUT_GUARD_BYTE = 0xFF
GUARD_BYTE = 0xA5
OUTPUT_BYTE = 0xFF


def _round_up(x, m):
    return (x + m - 1) // m * m


class Region:
    """One buffer of the call: `kind` in ("input", "workspace", "output"); [start, start + nbytes) from the arena's
    base; guards [front, start) and [start + nbytes, behind_end)."""

    def __init__(self, arena, name, kind, nbytes, dtype, shape):
        self.arena, self.name, self.kind, self.nbytes = arena, name, kind, int(nbytes)
        self.dtype, self.shape = np.dtype(dtype), tuple(shape)
        self.front = self.start = self.behind_end = None

    @property
    def end(self):
        return self.start + self.nbytes

    @property
    def ptr(self):
        """The address to hand to the call."""
        return self.arena.base_ptr + self.start

    @property
    def guard_byte(self):
        return INPUT_GUARD_BYTE if self.kind == "input" else GUARD_BYTE

    def value(self):
        """The body as it was at the last read(), as a NumPy array of the region's dtype and shape (a copy)."""
        raw = self.arena.now()[self.start:self.end]
        return raw.view(self.dtype).reshape(self.shape).copy()

    def raw(self):
        """The body's bytes at the last read() (a copy)."""
        return self.arena.now()[self.start:self.end].copy()

    def changed(self):
        """Whether any byte of the body differs from the image the arena was started from."""
        return bool((self.arena.now()[self.start:self.end] != self.arena.image[self.start:self.end]).any())


class Arena:
    def __init__(self, backend="torch"):
        assert backend in ("torch", "numpy")
        self.backend, self.regions, self.image = backend, [], None
        self._cursor, self._pending, self._now, self._store = 0, [], None, None

    # ---------------------------------------------------------------------------------------------- layout ---
    def _add(self, name, kind, nbytes, dtype, shape, body):
        assert self.image is None, "the arena is already committed"
        assert all(r.name != name for r in self.regions), name
        r = Region(self, name, kind, nbytes, dtype, shape)
        r.front = self._cursor
        r.start = _round_up(r.front + GUARD, ALIGN)
        r.behind_end = _round_up(r.end + GUARD, ALIGN)
        self._cursor = r.behind_end
        self.regions.append(r)
        self._pending.append(body)
        return r

    def add_input(self, name, array):
        a = np.ascontiguousarray(array)
        return self._add(name, "input", a.nbytes, a.dtype, a.shape, a.reshape(-1).view(np.uint8))

    def add_workspace(self, name, nbytes, fill):
        return self._add(name, "workspace", nbytes, np.uint8, (int(nbytes),), int(fill))

    def add_output(self, name, shape, dtype, init=None, fill=OUTPUT_BYTE):
        """An output of `shape` and `dtype`, every byte `fill` -- or holding `init`, for an output of which the call
        leaves some elements to the caller."""
        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        body = int(fill)
        if init is not None:
            body = np.ascontiguousarray(init, dtype=dtype).reshape(-1).view(np.uint8)
            assert body.size == nbytes
        return self._add(name, "output", nbytes, dtype, shape, body)

    def commit(self):
        """Build the byte image, allocate the arena and upload the image.  Returns self."""
        assert self.image is None and self.regions
        self.regions[-1].behind_end += SLACK
        image = np.empty(self.regions[-1].behind_end, np.uint8)
        for r, body in zip(self.regions, self._pending):
            image[r.front:r.behind_end] = r.guard_byte
            image[r.start:r.end] = body
        self.image, self._pending = image, None
        if self.backend == "numpy":
            self._store = image.copy()
            self.base_ptr = self._store.ctypes.data
        else:
            import torch
            self._store = torch.from_numpy(image).to("cuda")
            self.base_ptr = self._store.data_ptr()
            assert self.base_ptr % ALIGN == 0
        self._now = None
        return self

    def __getitem__(self, name):
        return next(r for r in self.regions if r.name == name)

    # ------------------------------------------------------------------------------------------ the bytes ---
    def reset(self, workspace_fill=None):
        """Put the image back; with `workspace_fill`, every workspace body (of the image too) takes that byte."""
        if workspace_fill is not None:
            for r in self.regions:
                if r.kind == "workspace":
                    self.image[r.start:r.end] = int(workspace_fill)
        if self.backend == "numpy":
            self._store[:] = self.image
        else:
            import torch
            self._store.copy_(torch.from_numpy(self.image))
        self._now = None

    def store(self):
        """The arena itself (a NumPy byte array or a torch.uint8 tensor): where a test plants its own writes."""
        return self._store

    def read(self):
        """Bring the arena's bytes back (the caller has synchronised the device).  Returns them."""
        self._now = self._store.copy() if self.backend == "numpy" else self._store.cpu().numpy()
        return self._now

    def now(self):
        return self._now if self._now is not None else self.read()

    def check(self):
        """Reads the arena and returns one entry per guard of which any byte changed:
            {"region": name, "side": "front" | "behind", "first": k, "last": k', "bytes": count}
        `first` and `last` are the offsets of the first and the last changed byte from the end of the body that the
        guard touches: behind the region 0 is the byte right after the body's last; in front -1 is the byte right before
        the body's first.  Empty when every guard holds what it was filled with."""
        now, found = self.read(), []
        for r in self.regions:
            for side, lo, hi, origin in (("front", r.front, r.start, r.start), ("behind", r.end, r.behind_end, r.end)):
                bad = np.flatnonzero(now[lo:hi] != self.image[lo:hi])
                if bad.size:
                    found.append({"region": r.name, "side": side, "first": int(bad[0]) + lo - origin,
                                  "last": int(bad[-1]) + lo - origin, "bytes": int(bad.size)})
        return found

    def changed_bodies(self):
        """Names of the workspace and output regions of which any byte differs from the image (a refused call must
        leave this empty)."""
        return [r.name for r in self.regions if r.kind != "input" and r.changed()]
