"""The dropout rule (csrc/dropout_rng.h) and the kernel selection (csrc/dropout_select.h) restated in numpy / plain Python for the
tests: Philox4x32-10, the keep decision of an element index, the mask of an (M, C) call, the expected output of kd_dropout_nhwc, and
which kernel a call runs.  tests/test_dropout_host.py holds both restatements to the compiled headers; tests/test_dropout_gpu.py
holds the kernels to them bit for bit."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = 0xFFFFFFFF

TPB, CAP, VEC_BYTES, BLOCK = 256, 2048, 16, 4
NAMES = ("dropout_block_kernel<float>", "dropout_vec_kernel<float, 4>", "dropout_block_kernel<bf16_t>", "dropout_vec_kernel<bf16_t, 8>")
F32, BF16 = 0, 1


def philox4x32_10(ctr, key):
    """ctr: 4 uint64 arrays (or ints) holding 32-bit words, key: 2 ints -> 4 uint64 arrays of 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(U32) for v in ctr]
    k0, k1 = int(key[0]) & U32, int(key[1]) & U32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(U32), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(U32)]
        k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
    return c


def words(seed, offset, idx):
    """The 32-bit word of every element index of `idx` (any integer array, values below 2^63)."""
    idx = np.asarray(idx, dtype=np.uint64)
    q = idx >> np.uint64(2)
    seed, offset = int(seed), int(offset)
    out = philox4x32_10((q & np.uint64(U32), q >> np.uint64(32), offset & U32, offset >> 32), (seed & U32, seed >> 32))
    sel = (idx & np.uint64(3)).astype(np.int64)
    return np.choose(sel, [np.broadcast_to(w, idx.shape) for w in out]).astype(np.uint64)


def params(p):
    """(threshold, scale) as ops.dropout_params computes them."""
    return int(p * 4294967296.0), np.float32(1.0 / (1.0 - p))


def keep(seed, offset, idx, threshold):
    return words(seed, offset, idx) >= np.uint64(threshold)


def mask(seed, offset, M, C, p):
    """Boolean (M, C) keep mask of a call: idx = m * C + c."""
    return keep(seed, offset, np.arange(M * C, dtype=np.uint64), params(p)[0]).reshape(M, C)


def apply_f32(x, kept, p):
    """y = keep ? x * scale : 0 in float32 for a float32 array."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(kept, x * params(p)[1], np.float32(0)).astype(np.float32)


def bf16_round(x):
    """float32 array -> the bf16 bit patterns (uint16) of round-to-nearest-even (finite values)."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def apply_bf16(bits, kept, p):
    """bf16 bit patterns in -> bf16 bit patterns out: the product in float32, rounded once."""
    return bf16_round(apply_f32(bf16_to_f32(bits), kept, p))


# ---- csrc/dropout_select.h
def vec_ok(dtype, C, x_ptr, ldx, y_ptr, ldy):
    v = VEC_BYTES // (2 if dtype == BF16 else 4)
    return C % v == 0 and ldx % v == 0 and ldy % v == 0 and x_ptr % 16 == 0 and y_ptr % 16 == 0


def grid(items):
    return max(1, min(CAP, -(-items // TPB)))


def predict(dtype, M, C, x_ptr, ldx, y_ptr, ldy):
    """(kernel name, channels per access, items, workgroups) of a call."""
    vec = vec_ok(dtype, C, x_ptr, ldx, y_ptr, ldy)
    v = VEC_BYTES // (2 if dtype == BF16 else 4) if vec else 1
    items = M * (C // v) if vec else -(-(M * C) // BLOCK)
    return NAMES[(2 if dtype == BF16 else 0) + (1 if vec else 0)], v, items, grid(items)
