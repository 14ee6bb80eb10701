"""A poisoning allocator for the scratch memory of the kernels (tests/test_scratch_gpu.py, test_scratch_host.py).

ops.py takes every buffer it hands the library without returning it from two helpers, _ws (bytes) and _scratch (typed), and keeps
two per-stream caches for the criteria (_ws_cache, _topk_ws).  poison() replaces the helpers for the length of a `with` block:
every buffer handed out is the middle of a larger allocation, GUARD bytes on each side, all of it pre-filled with one of FILLS.
A kernel whose result depends on what its scratch held shows as a result that differs between fills; a kernel that stores past
the bytes its kd_*_workspace() declared shows as a changed guard byte when the block ends.
"""
import contextlib
import sys
import zlib

import torch

GUARD = 4096            # a multiple of the caching allocator's 512-byte granule: the middle is aligned as a bare allocation is
FILLS = ("zero", "ones", "noise")       # 0x00; 0xFF (NaN as fp32 / bf16 / fp64, -1 as any integer); seeded bytes


def _gen(key):          # (as tests/_seeded.py seeds)
    g = torch.Generator()
    g.manual_seed(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    return g


def fill_bytes(fill, n, key):
    """The CPU uint8 pattern of `n` bytes of a fill."""
    if fill == "zero":
        return torch.zeros(n, dtype=torch.uint8)
    if fill == "ones":
        return torch.full((n,), 0xFF, dtype=torch.uint8)
    if fill == "noise":
        return torch.randint(0, 256, (n,), generator=_gen(key), dtype=torch.uint8)
    raise KeyError(fill)


class Buffer:
    """One buffer handed out: `whole` = front guard | `nbytes` of scratch | back guard, `entry` the ops function that asked."""

    def __init__(self, entry, whole, nbytes, pattern):
        self.entry, self.whole, self.nbytes = entry, whole, nbytes
        self.front, self.back = pattern[:GUARD].clone(), pattern[GUARD + nbytes:].clone()      # what the guards must still hold
        self.pattern = pattern

    @property
    def middle(self):
        return self.whole[GUARD:GUARD + self.nbytes]

    def first_damage(self):
        """Offset, relative to the first scratch byte, of the first guard byte that no longer holds the fill (None: intact)."""
        for base, want, got in ((-GUARD, self.front, self.whole[:GUARD]), (self.nbytes, self.back, self.whole[GUARD + self.nbytes:])):
            bad = (got.cpu() != want).nonzero()
            if bad.numel():
                return base + int(bad[0])
        return None

    def high_water(self):
        """One past the last scratch byte that differs from the fill (0: nothing written, or only bytes equal to the fill)."""
        bad = (self.middle.cpu() != self.pattern[GUARD:GUARD + self.nbytes]).nonzero()
        return int(bad[-1]) + 1 if bad.numel() else 0


class Poison:
    def __init__(self, ops, fill, key):
        self.ops, self.fill, self.key = ops, fill, key
        self.buffers = []

    count = property(lambda self: len(self.buffers))

    def _entry(self):
        """The outermost function of ops.py on the stack: the entry point the test called."""
        f, name = sys._getframe(1), "?"
        while f is not None:
            if f.f_code.co_filename == self.ops.__file__:
                name = f.f_code.co_name
            f = f.f_back
        return name

    def alloc(self, nbytes, device, entry=None):
        nbytes = int(nbytes)
        pattern = fill_bytes(self.fill, nbytes + 2 * GUARD, f"{self.key}:{self.count}")
        whole = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=device)
        whole.copy_(pattern)
        b = Buffer(entry or self._entry(), whole, nbytes, pattern)
        self.buffers.append(b)
        return b.middle

    def ws(self, nbytes, device, floor=16):
        return self.alloc(max(int(nbytes), floor), device)

    def scratch(self, shape, dtype, device):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = 1
        for d in shape:
            n *= d
        return self.alloc(n * torch.empty((), dtype=dtype).element_size(), device).view(dtype).view(shape)

    def seed_caches(self, nbytes, device):
        """Put one guarded buffer of `nbytes` into both criterion caches for `device`'s current stream: every criterion of the block
        then works in the same bytes, whatever the one before it left there."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())      # (the key ops.py uses: a tensor's .device)
        stream = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
        self.ops._ws_cache[(device, stream)] = self.alloc(nbytes, device, entry="loss_workspace (cache)")
        self.ops._topk_ws[(device, stream)] = self.alloc(nbytes, device, entry="topk_hint_mse (cache)")

    def assert_guards(self):
        for i, b in enumerate(self.buffers):
            at = b.first_damage()
            assert at is None, (f"{b.entry}: scratch buffer {i} of {b.nbytes} bytes ({self.fill} fill): the first changed guard byte is at offset {at} "
                                f"({'before the buffer' if at < 0 else f'{at - b.nbytes} past its last byte'})")


@contextlib.contextmanager
def poison(monkeypatch, ops, fill, key="scratch", seed_caches=None, device="cuda"):
    """While the block runs, ops._ws / ops._scratch hand out guarded memory pre-filled with `fill` and the criterion caches start
    empty (or, with seed_caches=nbytes, hold one guarded buffer of that size each).  Yields the Poison (its .buffers and .count);
    when the block ends without an exception every guard must still hold the fill; the caches are put back either way."""
    p = Poison(ops, fill, key)
    saved = dict(ops._ws_cache), dict(ops._topk_ws)
    with monkeypatch.context() as m:
        m.setattr(ops, "_ws", p.ws)
        m.setattr(ops, "_scratch", p.scratch)
        ops._ws_cache.clear()
        ops._topk_ws.clear()
        try:
            if seed_caches is not None:
                p.seed_caches(seed_caches, device)
            yield p
        finally:
            for cache, old in zip((ops._ws_cache, ops._topk_ws), saved):
                cache.clear()
                cache.update(old)
    p.assert_guards()
