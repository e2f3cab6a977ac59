"""The exact-operand ("f16x6") claim on paper: over which fp32 operands do three f16 pieces reproduce the value, where does the bf8 copy of
the third piece stop being exact, and is the bf8 re-arrangement of the weight blob the layout its docstring names?  All on the numpy
restatement tests/split_model.py -- no GPU, no library.  The constants asserted here are the ones robir_amd/precision.py and DESIGN
section 6 quote and the GPU tests import (tests/test_mlp_gpu.py holds the device's packing to the same model bit for bit,
tests/test_precision_gpu.py the kernels' error over the windows)."""
import numpy as np
import pytest
import torch

import split_model as sm

SPLITS = {"weight": sm.split_weight, "activation": sm.split_activation}


def _binade(e, rng, n=2048):
    """fp32 values of both signs with |v| in [2^e, 2^(e+1)), e = -149 .. 15: n random mantissas, the two edges and their neighbours"""
    if e < -126:                                                  # fp32 subnormals: the pattern is the mantissa
        lo = 1 << (e + 149)
        bits = np.concatenate([rng.integers(lo, 2 * lo, size=min(n, lo)), [lo, min(lo + 1, 2 * lo - 1), 2 * lo - 1]])
    else:
        base = (e + 127) << 23
        bits = np.concatenate([base + rng.integers(0, 1 << 23, size=n), [base, base + 1, base + (1 << 23) - 2, base + (1 << 23) - 1]])
    v = bits.astype(np.uint32).view(np.float32)
    assert np.all(np.abs(v) >= np.float32(2.0 ** e)) and np.all(np.abs(v.astype(np.float64)) < 2.0 ** (e + 1))
    return np.concatenate([v, -v])


@pytest.mark.parametrize("which", sorted(SPLITS))
def test_exactness_window(which):
    """Every fp32 binade from the smallest subnormal to 2^16: |v - (h + m 2^-11 + l 2^-22)| is ZERO for EXACT_MIN <= |v| <= 65504 and at most
    min(|v|, BELOW_WINDOW_ABS_ERR) below; the bound below is attained (it is not a loose one), and the window cannot be extended by a binade."""
    split = SPLITS[which]
    rng = np.random.default_rng(7)
    worst_below, worst_outside_binade = 0.0, None
    for e in range(-149, 16):
        v = _binade(e, rng)
        v = v[np.abs(v) <= np.float32(sm.F16_MAX)]
        h, m, l = split(v)
        for p in (h, m, l):
            assert np.all(np.isfinite(p.astype(np.float32))), (which, e)
        err = np.abs(sm.reconstruct(h, m, l) - v.astype(np.float64))
        if 2.0 ** e >= sm.EXACT_MIN:
            assert np.array_equal(sm.reconstruct(h, m, l), v.astype(np.float64)), (which, e, float(err.max()))
        else:
            assert np.all(err <= np.minimum(np.abs(v.astype(np.float64)), sm.BELOW_WINDOW_ABS_ERR)), (which, e, float(err.max()))
            worst_below = max(worst_below, float(err.max()))
            if err.max() > 0:
                worst_outside_binade = e                                     # e ascends: the last one is the highest inexact binade
    assert worst_below == sm.BELOW_WINDOW_ABS_ERR                            # attained
    assert 2.0 ** (worst_outside_binade + 1) == sm.EXACT_MIN                 # the binade right below the window is NOT exact
    # +-0, the largest half and the fp32 values right below it (the top of the clamp's binade)
    top = np.arange(np.float32(65472.0).view(np.uint32), np.float32(65504.0).view(np.uint32) + 1, dtype=np.uint32).view(np.float32)
    edge = np.concatenate([np.array([0.0, -0.0, sm.EXACT_MIN, -sm.EXACT_MIN], dtype=np.float32), top, -top])
    h, m, l = split(edge)
    assert np.array_equal(sm.reconstruct(h, m, l), edge.astype(np.float64))
    assert np.array_equal(h[:2].view(np.uint16), np.array([0x0000, 0x8000], dtype=np.uint16)) and not m[:2].any() and not l[:2].any()


def test_activation_split_clamp_binade():
    """[32768, 65504] exhaustively (every fp32 value): the round-toward-zero residual times 2048 exceeds 65504 for some of them, the m piece
    then CLAMPS at 65504 (round-toward-zero conversion: no infinity) and the l piece takes the rest -- the value is still exact.  Most of
    these under a round-to-nearest m would be infinity: the split relies on the clamp."""
    v = np.arange(np.float32(32768.0).view(np.uint32), np.float32(65504.0).view(np.uint32) + 1, dtype=np.uint32).view(np.float32)
    h, m, l = sm.split_activation(v)
    d = (v.astype(np.float64) - h.astype(np.float64)) * 2048.0
    clamped = d > sm.F16_MAX
    assert clamped.sum() > 1000
    assert np.all(m[clamped] == np.float16(sm.F16_MAX)) and np.isinf(sm.f16_rne(d[clamped].astype(np.float32))).sum() > 1000
    assert np.all(np.isfinite(l.astype(np.float32))) and float(np.abs(l.astype(np.float32)).max()) < sm.F16_MAX
    for sign in (1.0, -1.0):
        hh, mm, ll = sm.split_activation(v * np.float32(sign))
        assert np.array_equal(sm.reconstruct(hh, mm, ll), (v * np.float32(sign)).astype(np.float64))
    # and beyond the range: the h piece saturates at 65504 -- the pattern the kernels' range sentinel looks for -- from 65504 on, not before
    hs = sm.f16_rtz(np.array([65503.996, 65504.0, 65520.0, 1.0e6, 3.0e38], dtype=np.float32)).view(np.uint16)
    assert hs.tolist() == [0x7BFE, 0x7BFF, 0x7BFF, 0x7BFF, 0x7BFF]


@pytest.mark.parametrize("which", sorted(SPLITS))
def test_third_piece_survives_bf8_inside_its_window(which):
    """|v| >= 2^-14 (h a normal half), and as measured one binade further down to BF8_L_EXACT_MIN = 2^-15: the third piece has at most three
    significant bits and both bf8 conversions (truncation: activations in the kernel; round-to-nearest-even with saturation: weights in
    repack_x6_chunks_fp8) return it bit for bit.  BF8_L_FIRST_FAIL, one fp32 unit below, is the largest magnitude where they do not."""
    split = SPLITS[which]
    rng = np.random.default_rng(11)
    assert sm.BF8_L_EXACT_MIN <= 2.0 ** -14
    for e in range(-15, 16):
        v = _binade(e, rng, n=8192)
        v = v[np.abs(v) <= np.float32(sm.F16_MAX)]
        l = split(v)[2]
        pat = l.view(np.uint16)
        assert not np.any(pat & 0x00FF), (which, e)                         # three significant bits: the low byte is empty
        for conv in (sm.bf8_trunc, sm.bf8_rne_sat):
            assert np.array_equal(sm.bf8_decode(conv(l)).view(np.uint16), pat), (which, e, conv.__name__)
    # the whole binade below, every value: where does it first fail?
    hi = int(np.float32(sm.BF8_L_EXACT_MIN).view(np.uint32))
    v = np.arange(hi - (1 << 23), hi, dtype=np.uint32).view(np.float32)
    for sign in (1.0, -1.0):
        l = split(v * np.float32(sign))[2]
        for conv in (sm.bf8_trunc, sm.bf8_rne_sat):
            bad = sm.bf8_decode(conv(l)).view(np.uint16) != l.view(np.uint16)
            assert float(v[np.nonzero(bad)[0].max()]) == sm.BF8_L_FIRST_FAIL, (which, sign, conv.__name__)
    assert sm.BF8_L_FIRST_FAIL == float(np.nextafter(np.float32(sm.BF8_L_EXACT_MIN), np.float32(0)))


@pytest.mark.parametrize("which", sorted(SPLITS))
def test_bf8_form_below_its_window(which):
    """Below BF8_L_EXACT_MIN the operand as the bf8 form carries it -- h + m 2^-11 + bf8(l) 2^-22 -- is off by less than
    BF8_BELOW_WINDOW_ABS_ERR = 2^-38 in absolute terms (against 2^-47 for the six-product form); the bound is nearly attained by truncation
    (the activations' conversion) and half of it by round-to-nearest (the weights')."""
    split, conv, reach = SPLITS[which], {"activation": sm.bf8_trunc, "weight": sm.bf8_rne_sat}[which], {"activation": 0.99, "weight": 0.5}[which]
    rng = np.random.default_rng(13)
    worst = 0.0
    for e in range(-149, -15):
        v = _binade(e, rng, n=8192)
        h, m, l = split(v)
        err = np.abs(sm.reconstruct(h, m, sm.bf8_decode(conv(l))) - v.astype(np.float64))
        assert np.all(err < sm.BF8_BELOW_WINDOW_ABS_ERR) and np.all(err <= np.abs(v.astype(np.float64))), (which, e, float(err.max()))
        worst = max(worst, float(err.max()))
    assert reach * sm.BF8_BELOW_WINDOW_ABS_ERR <= worst


def test_bf8_conversions():
    """All 65536 half patterns: truncation is the top byte; round-to-nearest-even picks the nearer e5m2 neighbour (the even one on a tie),
    never turns a finite half into infinity, and keeps zeros, infinities and the sign."""
    pat = np.arange(1 << 16, dtype=np.uint16)
    h = pat.view(np.float16)
    fin = np.isfinite(h.astype(np.float32))
    t, r = sm.bf8_trunc(h), sm.bf8_rne_sat(h)
    assert np.array_equal(t, (pat >> 8).astype(np.uint8))
    assert np.all((r[fin] & 0x7F) <= 0x7B)
    assert np.array_equal(r[~fin & ((pat & 0x3FF) == 0)], t[~fin & ((pat & 0x3FF) == 0)])            # infinities stay
    x, lo = h[fin].astype(np.float64), sm.bf8_decode(t[fin]).astype(np.float64)                      # lo: the neighbour toward zero
    up_byte = t[fin].astype(np.int32) + 1
    can_up = (up_byte & 0x7F) <= 0x7B
    up = np.where(can_up, sm.bf8_decode(np.where(can_up, up_byte, 0).astype(np.uint8)).astype(np.float64), np.inf * np.sign(x + (x == 0)))
    got = sm.bf8_decode(r[fin]).astype(np.float64)
    dl, du = np.abs(x - lo), np.where(can_up, np.abs(up - x), np.inf)
    want = np.where(dl < du, lo, np.where(du < dl, up, np.where(t[fin] & 1, up, lo)))
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(x))
    # packing.repack_x6_chunks_fp8's own expression on every finite pattern (it is applied to uint32 copies of the patterns)
    p = pat.astype(np.uint32)
    b8 = ((p + 0x7F + ((p >> 8) & 1)) >> 8).astype(np.uint8)
    b8 = np.where(((p & 0x7C00) != 0x7C00) & ((b8 & 0x7F) >= 0x7C), (b8 & 0x80) | 0x7B, b8).astype(np.uint8)
    assert np.array_equal(b8[fin], r[fin])


@pytest.mark.parametrize("n_pad,k_pad", [(16, 32), (48, 96), (256, 256)])
def test_layout_map_is_a_bijection(n_pad, k_pad):
    """blob position -> (row, slot, piece) and back: every (row, slot, piece) and every bias has exactly one position, together they fill the blob."""
    is_bias, row, k, piece = sm.layout_x6(n_pad, k_pad)
    n = is_bias.size
    assert n == (n_pad // 16) * sm.chunk_halves(k_pad) and int(is_bias.sum()) == 2 * n_pad
    body = ~is_bias
    assert np.array_equal(sm.half_index(row[body], k[body], piece[body], k_pad), np.nonzero(body)[0])
    R, K, P = np.meshgrid(np.arange(n_pad), np.arange(k_pad), np.arange(3), indexing="ij")
    idx = sm.half_index(R, K, P, k_pad).reshape(-1)
    assert np.unique(idx).size == idx.size == int(body.sum()) and np.all(body[idx])
    assert np.array_equal(np.sort(np.concatenate([2 * sm.bias_index(np.arange(n_pad), k_pad), 2 * sm.bias_index(np.arange(n_pad), k_pad) + 1])),
                          np.nonzero(is_bias)[0])
    # what the layout means to the MFMA: a lane's 8 halves of a k-block are slots 4 g + 0..3 and 16 + 4 g + 0..3, its row is lane % 16
    assert sm.slot_of(2, 37, np.arange(8)).tolist() == [64 + 8 + i for i in range(4)] + [64 + 16 + 8 + i for i in range(4)]


@pytest.mark.parametrize("K,n_chunks", [(128, 3), (256, 4)])
def test_repack_x6_chunks_fp8_against_the_layout_map(K, n_chunks):
    """packing.repack_x6_chunks_fp8 on a CPU blob built by the model's layout map (weights over every binade, with biases, a tail of padding
    behind the chunks): the f16 h and m planes are moved, not changed; every h8 / l8 byte decodes to the model's bf8 value of the piece at the
    K position the docstring names; biases and padding are kept; no finite half becomes a bf8 infinity."""
    from robir_amd import packing
    rng = np.random.default_rng(100 + K)
    n = 16 * n_chunks
    W = sm.operand_matrix(rng, n - 3, K - 5)                         # ragged: three padding rows, five padding columns
    b = rng.standard_normal(n - 3).astype(np.float32)
    blob = sm.pack_layer_x6(W, b, n, K)
    tail = rng.standard_normal(64).astype(np.float32)
    src = np.concatenate([blob, tail])
    out = packing.repack_x6_chunks_fp8(torch.from_numpy(src.copy()), "cpu", ((K, n_chunks),))
    assert out.dtype == torch.float32 and out.shape == (src.size,)
    out = out.numpy()
    o16, o8 = out.view(np.uint16), out.view(np.uint8)
    assert np.array_equal(out[blob.size:].view(np.uint32), tail.view(np.uint32))                                          # padding kept
    bi = sm.bias_index(np.arange(n), K)
    assert np.array_equal(out[bi].view(np.uint32), np.concatenate([b, np.zeros(3, np.float32)]).view(np.uint32))         # biases kept
    h, m, l = (np.zeros((n, K), np.float16) for _ in range(3))
    h[:n - 3, :K - 5], m[:n - 3, :K - 5], l[:n - 3, :K - 5] = sm.split_weight(W)
    chunk, kb, lane, j = np.meshgrid(np.arange(n_chunks), np.arange(K // 32), np.arange(64), np.arange(8), indexing="ij")
    row, k = 16 * chunk + lane % 16, sm.slot_of(kb, lane, j)
    for piece, plane in ((0, h), (1, m)):                                                                                 # f16 planes: moved
        assert np.array_equal(o16[sm.f16_plane_index(chunk, kb, piece, lane, j, K)], plane[row, k].view(np.uint16)), piece
    j8, r = 2 * (kb % 4) + j // 4, j % 4                             # byte 4 j8 + r <- half 4 (j8 % 2) + r of k-block 4 G + j8 / 2
    assert np.array_equal(4 * (j8 % 2) + r, j) and np.array_equal(4 * (kb // 4) + j8 // 2, kb)
    for which, plane in ((0, h), (1, l)):
        got = o8[sm.bf8_byte_index(chunk, kb // 4, which, lane, j8, r, K)]
        assert np.array_equal(got, sm.bf8_rne_sat(plane[row, k])), which
        assert not np.any((got & 0x7F) >= 0x7C)                                                                           # no infinity, no NaN
        inside = np.abs(sm.reconstruct(h, m, l)[row, k]) >= sm.BF8_L_EXACT_MIN
        if which == 1:                                               # inside its window the l piece survives the copy bit for bit
            assert np.array_equal(sm.bf8_decode(got[inside]).view(np.uint16), plane[row, k][inside].view(np.uint16))
    # every byte of the blob is accounted for: the model's own restatement of the whole re-arrangement gives the same array
    assert np.array_equal(sm.repack_fp8(src, ((K, n_chunks),)).view(np.uint32), out.view(np.uint32))
    assert float(np.abs(h.astype(np.float32)).max()) > 60000.0 and np.any((sm.bf8_rne_sat(h) & 0x7F) == 0x7B)           # saturation was exercised


def test_pack_layer_model_perm_and_padding():
    """the model's own pack (what tests/test_mlp_gpu.py compares the device with): perm entries of -1 or beyond k_in and rows beyond n_out give
    zero halves, a slot holds the pieces of column perm[slot], the bias floats are b 2^s."""
    rng = np.random.default_rng(5)
    W = sm.operand_matrix(rng, 17, 39, top=sm.F16_MAX / 256)
    b = rng.standard_normal(17).astype(np.float32)
    perm = rng.permutation(64).astype(np.int64) - 10                 # -10 .. 53: negative and >= 39 entries
    blob = sm.pack_layer_x6(W, b, 32, 64, perm, 8)
    u16 = blob.view(np.uint16)
    is_bias, row, k, piece = sm.layout_x6(32, 64)
    body = np.nonzero(~is_bias)[0]
    kin = perm[k[body]]
    live = (row[body] < 17) & (kin >= 0) & (kin < 39)
    assert not u16[body[~live]].any()
    pieces = np.stack([p.view(np.uint16) for p in sm.split_weight(W, 8)])
    assert np.array_equal(u16[body[live]], pieces[piece[body[live]], row[body[live]], kin[live]])
    assert np.array_equal(blob[sm.bias_index(np.arange(32), 64)], np.concatenate([b * np.float32(256.0), np.zeros(15, np.float32)]))
    h, m, l = sm.split_weight(W, 8)
    assert np.array_equal(sm.reconstruct(h, m, l)[np.abs(W) * 256 >= sm.EXACT_MIN], (W.astype(np.float64) * 256)[np.abs(W) * 256 >= sm.EXACT_MIN])
