"""A plain numpy restatement of the exact-operand ("f16x6") operand handling: what the HIP code is MEANT to compute, instruction by
instruction, so that tests can hold the device to it bit for bit (tests/test_split_cpu.py: the model's own properties, no GPU;
tests/test_mlp_gpu.py: rb_pack_layer_x6 and pack_vis_split's bf8 blob against it; tests/test_precision_gpu.py: the windows below).

  split_weight      csrc/pack.hip k_pack_layer_x6: w 2^s = h + m 2^-11 + l 2^-22, three round-to-nearest casts, residuals in fp32
  split_activation  csrc/x6_ring.h sx_split_pair: h, m by v_cvt_pkrtz (round toward zero, finite values clamp at 65504), l by
                    v_fma_mixlo_f16 (round to nearest even); f16 subnormals carried, nothing flushed
  bf8_trunc         the activations' bf8 (e5m2) copies in csrc/vis_diffuse_x6t.hip: the top byte of the f16 pattern (v_perm_b32)
  bf8_rne_sat       the weights' bf8 copies in packing.repack_x6_chunks_fp8: round to nearest even, a finite half never becomes infinity
  half_index / layout_x6 / pack_layer_x6   the chunk layout of rb_pack_layer_x6, both directions
  bf8_byte_index / repack_fp8              the layout of packing.repack_x6_chunks_fp8

The windows (asserted as measured by tests/test_split_cpu.py; quoted by robir_amd/precision.py and DESIGN section 6):
"""
import numpy as np

F16_MAX = 65504.0
# The three pieces reproduce an fp32 value EXACTLY for EXACT_MIN <= |v| <= F16_MAX, and for v = +-0 (both splits).  The lower end is where
# the value's last bit (2^-23 |v|) meets the last bit the l piece can hold, 2^-24 (smallest f16 subnormal) x 2^-22 = 2^-46.
EXACT_MIN = 2.0 ** -23
# Below EXACT_MIN: |v - (h + m 2^-11 + l 2^-22)| <= min(|v|, BELOW_WINDOW_ABS_ERR): half a unit of that last bit (7.1e-15).
BELOW_WINDOW_ABS_ERR = 2.0 ** -47
# The bf8 (e5m2) copy of the third piece (l of a weight, xl of an activation) is bit-exact for BF8_L_EXACT_MIN <= |v| <= F16_MAX: there h keeps
# at least 10 significant bits and m 11, so the third piece has at most three, which is what e5m2 holds.  Below, h is a deeper f16
# subnormal, the third piece takes up to 11 bits and its bf8 copy drops all but three of them.  BF8_L_FIRST_FAIL is the largest fp32
# magnitude whose third piece does not survive (either split, either conversion): one fp32 unit below 2^-15.
BF8_L_EXACT_MIN = 2.0 ** -15
BF8_L_FIRST_FAIL = float(np.uint32(0x37FFFFFF).view(np.float32))
# Below BF8_L_EXACT_MIN the value as the bf8 form carries it, h + m 2^-11 + bf8(l) 2^-22, is off by less than BF8_BELOW_WINDOW_ABS_ERR (three
# leading bits of a third piece whose last bit is 2^-46: truncation, activations, reaches 0.998 of it; round to nearest, weights, half).
BF8_BELOW_WINDOW_ABS_ERR = 2.0 ** -38


# ------------------------------------------------------------------------------------------------------------------ casts
def f16_rne(x):
    """fp32 -> f16, round to nearest even; beyond the range -> infinity; subnormals kept (the compiler's (_Float16) cast)."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16)


def f16_rtz(x):
    """fp32 -> f16, round toward zero (v_cvt_pkrtz_f16_f32): a finite value beyond the range clamps to +-65504, subnormals kept."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(x.astype(np.float64))          # rounded away from zero (infinity included)
    over &= np.isfinite(x)
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float16)


def _f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ splits
def split_weight(w, scale_log2=0):
    """k_pack_layer_x6: v = w 2^s (fp32); h = f16(v); r1 = (v - h) 2048; m = f16(r1); r2 = (r1 - m) 2048; l = f16(r2).  -> f16 arrays"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.asarray(w, dtype=np.float32) * np.float32(2.0 ** scale_log2)
        h = f16_rne(v)
        r1 = (v - h.astype(np.float32)) * np.float32(2048.0)
        m = f16_rne(r1)
        r2 = (r1 - m.astype(np.float32)) * np.float32(2048.0)
        return h, m, f16_rne(r2)


def split_activation(v):
    """sx_split_pair: h = rtz(v); d = fma(h, -2048, v 2048); m = rtz(d); l = f16_rne(fma(m, -2048, d 2048)).  -> f16 arrays"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = f16_rtz(v)
        s = v * np.float32(2048.0)
        d = _f32(s.astype(np.float64) - h.astype(np.float64) * 2048.0)           # one rounding, like the fused multiply-add
        m = f16_rtz(d)
        e = d * np.float32(2048.0)
        r = _f32(e.astype(np.float64) - m.astype(np.float64) * 2048.0)
        return h, m, f16_rne(r)


def reconstruct(h, m, l):
    """h + m 2^-11 + l 2^-22 in float64 (exact: the pieces span fewer than 53 bits)"""
    return h.astype(np.float64) + m.astype(np.float64) * 2.0 ** -11 + l.astype(np.float64) * 2.0 ** -22


# ------------------------------------------------------------------------------------------------------------------ bf8 (e5m2)
def bf8_trunc(h16):
    """f16 -> e5m2 byte by truncation: the top byte of the pattern"""
    return (np.asarray(h16, dtype=np.float16).view(np.uint16) >> 8).astype(np.uint8)


def bf8_rne_sat(h16):
    """f16 -> e5m2 byte, round to nearest even; a finite half that would round up to infinity saturates at the largest finite e5m2"""
    p = np.asarray(h16, dtype=np.float16).view(np.uint16).astype(np.uint32)
    mag = p & 0x7FFF
    lower, rest = mag >> 8, mag & 0xFF
    up = (rest > 0x80) | ((rest == 0x80) & ((lower & 1) == 1))
    b = lower + up
    finite = (mag & 0x7C00) != 0x7C00
    b = np.where(finite & (b >= 0x7C), 0x7B, b)
    return (b | ((p >> 8) & 0x80)).astype(np.uint8)


def bf8_decode(b8):
    """e5m2 byte -> its value as f16 (the byte is the top byte of that half)"""
    return (np.asarray(b8, dtype=np.uint8).astype(np.uint16) << 8).view(np.float16)


# ------------------------------------------------------------------------------------------------------------------ rb_pack_layer_x6
def chunk_halves(k_pad):
    """uint16 elements of one 16-row chunk: 16 bias floats, then [k-block][h | m | l][lane 64][8 halves]"""
    return 2 * (16 + 24 * k_pad)


def half_index(row, k, piece, k_pad):
    """(output row, packed K slot, piece 0 = h / 1 = m / 2 = l) -> position of that half in the blob viewed as uint16"""
    row, k, piece = np.asarray(row), np.asarray(k), np.asarray(piece)
    jb, r16, kb, kk = row // 16, row % 16, k // 32, k % 32
    g = np.where(kk < 16, kk // 4, (kk - 16) // 4)
    j = np.where(kk < 16, kk % 4, 4 + (kk - 16) % 4)              # which of the lane's 8 halves
    lane = 16 * g + r16
    return jb * chunk_halves(k_pad) + 32 + ((kb * 3 + piece) * 64 + lane) * 8 + j


def bias_index(row, k_pad):
    """output row -> position of its bias in the blob viewed as float32"""
    row = np.asarray(row)
    return (row // 16) * (chunk_halves(k_pad) // 2) + row % 16


def layout_x6(n_pad, k_pad):
    """The other direction: for every uint16 position of the blob -> (is_bias, row, k, piece); row / k / piece are -1 on the bias floats."""
    ch = chunk_halves(k_pad)
    i = np.arange((n_pad // 16) * ch)
    jb, o = i // ch, i % ch
    is_bias = o < 32
    q = np.maximum(o - 32, 0)
    j, lane, kp = q % 8, (q // 8) % 64, q // 512
    kb, piece = kp // 3, kp % 3
    g = lane // 16
    k = 32 * kb + np.where(j < 4, 4 * g + j, 16 + 4 * g + (j - 4))
    row = jb * 16 + lane % 16
    neg = -np.ones_like(i)
    return is_bias, np.where(is_bias, neg, row), np.where(is_bias, neg, k), np.where(is_bias, neg, piece)


def pack_layer_x6(W, b, n_pad, k_pad, perm=None, scale_log2=0):
    """rb_pack_layer_x6 -> the blob as a float32 array.  W [n_out, k_in] fp32, b [n_out] or None; packed slot k holds input column perm[k]
    (k itself without perm); slots whose column is negative or >= k_in, and rows >= n_out, are zero halves; bias floats are b 2^s (0 beyond)."""
    W = np.asarray(W, dtype=np.float32)
    n_out, k_in = W.shape
    pieces = np.stack([p.view(np.uint16) for p in split_weight(W, scale_log2)])           # [3, n_out, k_in]
    kin = np.arange(k_pad) if perm is None else np.asarray(perm, dtype=np.int64)
    assert kin.shape == (k_pad,)
    ok = (kin >= 0) & (kin < k_in)
    out = np.zeros((n_pad // 16) * chunk_halves(k_pad), dtype=np.uint16)
    rows, ks = np.meshgrid(np.arange(n_out), np.nonzero(ok)[0], indexing="ij")
    for piece in range(3):
        out[half_index(rows, ks, piece, k_pad)] = pieces[piece][rows, kin[ks]]
    out = out.view(np.float32)
    if b is not None:
        with np.errstate(over="ignore"):
            out[bias_index(np.arange(n_out), k_pad)] = np.asarray(b, dtype=np.float32) * np.float32(2.0 ** scale_log2)
    return out


# ------------------------------------------------------------------------------------------------------------------ repack_x6_chunks_fp8
def f16_plane_index(chunk, kb, piece, lane, j, K):
    """bf8 layout: position (uint16 view) of half j of `lane` in the f16 plane `piece` (0 = h, 1 = m) of k-block kb.  Per group of 128 K
    (12 KB): [k-block 0..3][h | m][lane][8 halves] (8 KB), then the h8 bytes (2 KB), then the l8 bytes (2 KB)."""
    G, kk = np.asarray(kb) // 4, np.asarray(kb) % 4
    return chunk * chunk_halves(K) + 32 + G * 6144 + ((kk * 2 + piece) * 64 + lane) * 8 + j


def bf8_byte_index(chunk, G, which, lane, j8, r, K):
    """bf8 layout: position (uint8 view) of byte 4 j8 + r of `lane`'s 32 bytes of group G; which = 0: h8, 1: l8.  The 32 bytes are two
    planes of 16 ([plane j8 / 4][lane][16 bytes]); the byte is the bf8 copy of half 4 (j8 % 2) + r of k-block 4 G + j8 / 2."""
    base = 2 * (chunk * chunk_halves(K) + 32 + G * 6144 + 4096 + which * 1024)
    return base + ((np.asarray(j8) // 4) * 64 + lane) * 16 + 4 * (np.asarray(j8) % 4) + r


def slot_of(kb, lane, j):
    """the packed K slot that half j of `lane` in k-block kb holds (the inverse of half_index's column part)"""
    g = np.asarray(lane) // 16
    j = np.asarray(j)
    return 32 * np.asarray(kb) + np.where(j < 4, 4 * g + j, 16 + 4 * g + (j - 4))


def repack_fp8(blob, layout):
    """packing.repack_x6_chunks_fp8 restated through the index maps above: blob (float32 array of rb_pack_layer_x6 chunks; `layout` = runs of
    (K, number of chunks)) -> same-sized float32 array in the bf8 layout."""
    src = np.asarray(blob, dtype=np.float32).view(np.uint16)
    out16 = src.copy()
    out8 = out16.view(np.uint8)
    pos = 0
    for K, nch in layout:
        ch = chunk_halves(K)
        lane, j = np.meshgrid(np.arange(64), np.arange(8), indexing="ij")
        for c in range(nch):
            s = src[pos:pos + ch]
            o16, o8 = out16[pos:pos + ch], out8[2 * pos:2 * (pos + ch)]
            for kb in range(K // 32):
                at = lambda piece: s[32 + ((kb * 3 + piece) * 64 + lane) * 8 + j]          # noqa: E731
                for piece in (0, 1):
                    o16[f16_plane_index(0, kb, piece, lane, j, K)] = at(piece)
                for which, piece in ((0, 0), (1, 2)):
                    j8, r = 2 * (kb % 4) + j // 4, j % 4
                    o8[bf8_byte_index(0, kb // 4, which, lane, j8, r, K)] = bf8_rne_sat(at(piece).view(np.float16))
            pos += ch
    return out16.view(np.float32)


# ------------------------------------------------------------------------------------------------------------------ test operands
def operand_matrix(rng, n_out, k_in, top=F16_MAX):
    """[n_out, k_in] fp32 weights over the whole operand range: exponents uniform over every binade from the fp32 subnormals to just under
    `top` (a power of two times 65504), both signs, and -- as far as the matrix has room -- +-0, the largest magnitude and the window edges."""
    e = rng.integers(-149, int(np.floor(np.log2(top))) + 1, size=(n_out, k_in))
    lim = top * (1 - 2.0 ** -12)
    W = np.ldexp(1.0 + rng.random((n_out, k_in)), e) * rng.choice([-1.0, 1.0], size=(n_out, k_in))
    W = np.clip(W, -lim, lim).astype(np.float32)
    flat = W.reshape(-1)
    special = np.array([0.0, -0.0, lim, -lim, 65472.0 * top / F16_MAX, EXACT_MIN, BF8_L_EXACT_MIN, BF8_L_FIRST_FAIL, 2.0 ** -14, 2.0 ** -24,
                        2.0 ** -149], dtype=np.float32)[:flat.size]
    flat[rng.choice(flat.size, size=special.size, replace=False)] = special
    return W
