"""What the GPU test modules share: the torch_gpu fixture, the library and stream handles, the guarded device buffer, the bit
comparisons and the checked call behind every instance table (LaunchLog).  A plain module: import from it what a test needs
(the fixture as `from gpu_harness import torch_gpu  # noqa: F401`)."""
import ctypes as C

import numpy as np
import pytest

FILL = 0xA5                      # sentinel byte of every buffer
GUARD = 256                      # bytes before and after a buffer's payload (keeps the payload 256-byte aligned)
SENT16 = np.frombuffer(bytes([FILL] * 2), np.uint16)[0]
SENT32 = np.frombuffer(bytes([FILL] * 4), np.uint32)[0]


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from s2_emit import _native as nat
    nat.load()
    return torch


def lib():
    from s2_emit import _native as nat
    return nat.load()


def stream(torch):
    from s2_emit import _engine as eng
    return eng._stream(torch)


class Buf:
    """`nbytes` of device memory `off` bytes past a 256-byte boundary, sentinel-filled, between two sentinel guard zones."""

    def __init__(self, torch, nbytes, off=0, data=None):
        self.torch, self.nbytes, self.lo = torch, int(nbytes), GUARD + off
        self.t = torch.full((GUARD + off + self.nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 256 == 0
        if data is not None:
            self.put(data)

    def put(self, data, at=0):
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        assert at + raw.size <= self.nbytes
        self.t[self.lo + at: self.lo + at + raw.size] = self.torch.from_numpy(raw.copy()).cuda()

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.lo)

    def get(self, dtype):
        """The payload as `dtype` (host copy), after checking that nothing outside it was written."""
        self.torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        assert (h[:self.lo] == FILL).all() and (h[self.lo + self.nbytes:] == FILL).all(), "write outside the buffer"
        return h[self.lo: self.lo + self.nbytes].copy().view(dtype)


def bits_equal(got, ref, what):
    """Both as float32: the same shape, NaN in the same places, every other element the same bits."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaN positions differ ({int(gn.sum())} vs {int(rn.sum())})"
    bad = got.view(np.uint32)[~gn] != ref.view(np.uint32)[~rn]
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ, first {got[~gn][bad][:4]} vs {ref[~rn][bad][:4]}"


def same_bits(got, ref, what):
    """The same in got's dtype (4 or 8 bytes wide)."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref, dtype=got.dtype)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    iv = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaN positions differ ({int(gn.sum())} vs {int(rn.sum())})"
    bad = (got.view(iv) != ref.view(iv)) & ~gn
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first {got[bad][:4]} vs {ref[bad][:4]}"


# ---- the documented summation tree (csrc/hsr_tree_dev.h), written out in NumPy: float64, one rounding per add ----------------------
def butterfly64(v):
    """The xor butterfly 32, 16, .., 1 over 64 entries (axis 0): wave_sum / butterfly_tree<64>; every lane's result is the same."""
    v = np.asarray(v, np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ off]
    return v[0]


def slot_tree(col):
    """A slot reduction: lane l adds slots l, l + 64, ... in order from 0.0 (lane_slot_sum); then the xor butterfly over the 64
    lane sums.  col: (slots,) or (slots, ...) - every trailing element is a sum of its own."""
    col = np.asarray(col, np.float64)
    v = np.zeros((64,) + col.shape[1:])
    for lane in range(64):
        s = np.zeros(col.shape[1:])
        for i in range(lane, len(col), 64):
            s = s + col[i]
        v[lane] = s
    return butterfly64(v)


def thread_sums(terms, ok, owned):
    """Per-thread accumulation of a 256-thread moments kernel: thread t starts every sum at 0.0 and adds, in order, the terms of
    the pixels owned[0][t], owned[1][t], ... that are `ok`.  terms (npix, M) float64 (every product already rounded on its own:
    the library is built without contraction), ok (npix,) bool, owned (passes, 256) pixel indices, -1 = none.  -> (256, M)."""
    acc = np.zeros((256, terms.shape[1]))
    for sel in owned if len(terms) else ():                          # an empty slot: every sum stays 0.0
        use = (sel >= 0) & ok[np.maximum(sel, 0)]
        with np.errstate(invalid="ignore", over="ignore"):
            acc = np.where(use[:, None], acc + terms[np.maximum(sel, 0)], acc)
    return acc


def wave_tree(acc):
    """The workgroup join (block_join4): acc (256, ...) per-thread sums -> xor butterfly 32..1 over each wave's 64 lanes, then the
    four wave sums in order, ((w0 + w1) + w2) + w3."""
    acc = np.asarray(acc, np.float64)
    w = [butterfly64(acc[64 * k: 64 * k + 64]) for k in range(4)]
    return ((w[0] + w[1]) + w[2]) + w[3]


class LaunchLog:
    """A family's launch record (the hsr_*_last_launch named `reader_name`) as one test module uses it; `seen` collects every
    kernel name its checked calls recorded.  joined: read() splits the record into the list of its names."""
    CAP = 2048

    def __init__(self, reader_name, joined=False):
        self.reader_name, self.joined, self.seen = reader_name, joined, set()

    def _read(self):
        buf = C.create_string_buffer(b"\x7f" * (self.CAP - 1), self.CAP)
        return getattr(lib(), self.reader_name)(buf, self.CAP), buf.value.decode()

    def read(self):
        """The record since the last read - None when nothing was launched - and clears it."""
        filled, text = self._read()
        if filled != 1:
            return None
        return text.split("; ") if self.joined else text

    def clear(self):
        getattr(lib(), self.reader_name)(None, 0)

    def call(self, expect, fn, *args):
        """Run an entry point that must succeed and record exactly `expect`; None: it launches nothing."""
        self.clear()
        rc = fn(*args)
        assert rc == 0, (rc, lib().hsr_last_error())
        got = self.read()
        assert got == expect, (got, expect)
        assert self._read() == (0, "")                                       # cleared by the read
        if got is not None:
            self.seen.update(got if self.joined else got.split("; "))

    def refused(self, fn, *args):
        """Run an entry point that must refuse its arguments: an error code and text, and no launch."""
        self.clear()
        rc = fn(*args)
        got = self.read()
        assert rc != 0 and got is None and lib().hsr_last_error(), (rc, got)
