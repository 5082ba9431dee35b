"""Each Mimi codec kernel, alone, against a float64 evaluation of its own definition.

The operations run through the lab door (csrc/mimi_lab.hip: mimi_lab_conv1d / _convtr / _linear /
_layernorm / _rvq_encode) on seeded host arrays; mimi_lab_plan reports which kernel, split-K factor and fold the launcher
takes for the geometry -- the launchers' own function, so the coverage asserted here is the coverage run.

Reference: plain float64 numpy of the definitions in csrc/mimi_kernels.h -- the im2col product for the convs,
the phase form for the k = 2 s transposed convs, x @ W.T for the linears.

Unit and bar (as helpers.linear_f64_bar): per output, |got - float64| / S with S = the sum of |a||b| over that
output's products (plus the absolute values of the bias, residual or accumulated-onto terms added to it).
Bar = 1.5 x the largest error, in that unit, of a left-to-right float32 accumulation of the same float32
products (then the same added terms, in the engine's order), over every output too -- computed each run from
numpy alone.  Outputs that pass through ELU / GELU: the float64 function on
both sides (the float32 side rounded to float32 again, as any stored output is).  ELU-input cases keep
K >= 63, so that the accumulation the bar models, not the last bit of expm1f, is what is measured.
Every element of every output (y, y2, the accumulated conv-layout target) is compared -- no averages -- and
every element outside the addressed region must still hold the sentinel.
"""
import math

import numpy as np
import pytest

from helpers import linear_err

pytestmark = pytest.mark.gpu

SENT = np.float32(-7777.25)
GEMV, G64, WIDE = 0, 1, 2
F64 = np.float64


# ----------------------------------------------------------------------------- the lab door
def _L():
    from csm_mlx import _lib
    return _lib, _lib.lib()


def _i32(v):
    return np.ascontiguousarray(v, np.int32)


def plan(op, geo):
    _lib, L = _L()
    g, out = _i32(geo), np.zeros(4, np.int32)
    _lib.check(L.mimi_lab_plan(op, _lib.ptr(g), len(g), _lib.ptr(out)))
    return dict(kernel=int(out[0]), bm=int(out[1]), ks=int(out[2]), fold=int(out[3]))


def _p(a):
    _lib, _ = _L()
    return None if a is None else _lib.ptr(a)


def elu64(v):
    v = np.asarray(v, F64)
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))


def gelu64(v, erf):
    v = np.asarray(v, F64)
    if erf:
        return 0.5 * v * (1 + np.vectorize(math.erf)(v / math.sqrt(2)))
    return 0.5 * v * (1 + np.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)))


def acts(rng, shape):
    """Seeded normals, about a third negative."""
    return (rng.standard_normal(shape) + 0.43).astype(np.float32)


def lr_sum(a, b):
    """a (..., R, K), b (C, K) float32: the left-to-right float32 accumulation of the float32 products
    a[..., r, k] * b[c, k], k = 0, 1, 2, ... -> (..., R, C).  Every output, so that the bar's maximum is taken
    over the same population as the engine's (a sampled bar sat 2 % under a 10-term sum's largest error)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros(a.shape[:-1] + (b.shape[0],), np.float32)
    for k in range(a.shape[-1]):
        acc = acc + a[..., k, None] * b[:, k]
    return acc


def check(name, got, ref64, S, lr_post):
    """Every output: got, its float64 value, its unit S and the left-to-right float32 evaluation."""
    bar = 1.5 * float(linear_err(lr_post, ref64, S))
    err = float(linear_err(got, ref64, S))
    print(f"{name}: err {err:.3e} bar {bar:.3e} ratio {err / bar:.2f}")
    assert bar > 0
    assert err <= bar, f"{name}: {err:.3e} > {bar:.3e} at {np.unravel_index(np.argmax(np.abs(got - ref64) / np.maximum(S, 1e-300)), got.shape)}"


def sentinel_intact(buf, idx, name):
    mask = np.ones(buf.shape, bool)
    mask[idx.reshape(-1)] = False
    bad = np.flatnonzero(mask & (buf.view(np.uint32) != SENT.view(np.uint32)))
    assert bad.size == 0, f"{name}: {bad.size} stores outside the addressed region, first at {bad[:5].tolist()}"


# ----------------------------------------------------------------------------- conv1d
def conv_out_len(T, k_eff, stride):
    """Output steps of a causal conv whose last frame is completed by right "extra" padding."""
    pad = k_eff - stride
    extra = (math.ceil((T - k_eff + pad) / stride + 1) - 1) * stride + (k_eff - pad) - T
    return (T + pad + extra - k_eff) // stride + 1


def conv(name, Cin, k, Cout, B=1, Tin=None, stride=1, dil=1, replicate=0, elu_in=0, elu_out=0, y2=0, bias=1, resid=0,
         x_off=0, x_gap=0, y_gap=0, r_off=0, r_gap=0, window=None, expect=None):
    """Encoder form (Tin given): pad_l = k_eff - stride, Tout = the causal conv's length with the right extra
    padding.  window = (n, P_next): the decoder's window form -- pad_l 0, Tin = (k - 1) dil + n, Tout = n, the
    output at offset P_next of rows P_next + n long.  *_gap: unused floats between channel rows."""
    k_eff = (k - 1) * dil + 1
    if window:
        Tout, y_off = window
        Tin, pad_l = k_eff - 1 + Tout, 0
    else:
        pad_l, y_off = k_eff - stride, 0
        Tout = conv_out_len(Tin, k_eff, stride)
    y_cs = y_off + Tout + y_gap
    x_cs = x_off + Tin + x_gap
    r_cs = r_off + Tout + r_gap
    return dict(name=name, op=0, Cin=Cin, Tin=Tin, x_bstride=Cin * x_cs + 3 * bool(x_gap), x_off=x_off, x_cstride=x_cs,
                Cout=Cout, k=k, stride=stride, dil=dil, pad_l=pad_l, replicate=replicate, elu_in=elu_in, Tout=Tout,
                y_bstride=Cout * y_cs + 5 * bool(y_gap), y_cstride=y_cs, y_off=y_off, r_bstride=Cout * r_cs, r_cstride=r_cs,
                r_off=r_off, B=B, elu_out=elu_out, y2=y2, bias=bias, resid=resid, expect=expect)


CONV_GEO = ("Cin", "Tin", "x_bstride", "x_off", "x_cstride", "Cout", "k", "stride", "dil", "pad_l", "replicate", "elu_in",
            "Tout", "y_bstride", "y_cstride", "y_off", "r_bstride", "r_cstride", "r_off", "B", "elu_out")


def P(kernel, ks=1, fold=0, bm=0):
    return dict(kernel=kernel, bm=bm, ks=ks, fold=fold)


CONV_CASES = [
    conv("k7_cin1", 1, 7, 8, Tin=70, expect=P(G64)),                                   # K = 7 < one 16-step
    conv("ragged_mnk", 9, 7, 65, Tin=65, elu_in=1, expect=P(G64)),                    # K = 63
    conv("ks2_partial", 21, 7, 64, Tin=64, elu_in=1, elu_out=1, expect=P(G64, ks=2)),  # K = 147: last slice partial
    conv("ks4", 40, 7, 64, Tin=64, y2=1, expect=P(G64, ks=4)),                        # K = 280
    conv("ks8", 74, 7, 64, Tin=64, expect=P(G64, ks=8)),                              # K = 518, not a multiple of 16
    conv("ks16", 147, 7, 64, Tin=30, expect=P(G64, ks=16)),                           # K = 1029
    conv("ks32", 512, 7, 64, Tin=2, expect=P(G64, ks=32)),                            # K = 3584
    # strided encoder form: k = 2 r, stride r, Tin no multiple of r (the right extra padding reads past the input)
    conv("enc_r4", 12, 8, 24, Tin=4 * 33 + 1, stride=4, elu_in=1, expect=P(G64)),
    conv("enc_r5", 13, 10, 24, Tin=5 * 30 + 2, stride=5, elu_in=1, y2=1, expect=P(G64, ks=2)),
    conv("enc_r6", 12, 12, 24, Tin=6 * 20 + 5, stride=6, elu_in=1, elu_out=1, expect=P(G64, ks=2)),
    conv("enc_r8", 8, 16, 70, Tin=8 * 17 + 3, stride=8, elu_in=1, x_off=1, x_gap=2, expect=P(G64, ks=2)),
    # downsample form: stride 2, k 4, replicate padding, odd Tin; B = 1 (b4k path), B = 3 (folded: kcontig off)
    conv("down_b1", 24, 4, 24, Tin=51, stride=2, replicate=1, bias=0, expect=P(G64)),
    conv("down_b3", 24, 4, 24, B=3, Tin=51, stride=2, replicate=1, bias=0, expect=P(G64, fold=26)),
    conv("down_b3_long", 24, 4, 24, B=3, Tin=135, stride=2, replicate=1, bias=0, expect=P(G64)),   # Tout 68: not folded
    # decoder window form
    conv("win_n2_b3", 24, 7, 40, B=3, window=(2, 2), elu_in=1, expect=P(G64, ks=2, fold=2)),
    conv("win_n6_b11", 24, 3, 40, B=11, window=(6, 1), dil=1, elu_in=1, elu_out=1, expect=P(G64, fold=6)),
    conv("win_xoff1", 24, 7, 40, B=2, window=(9, 0), x_off=1, x_gap=2, expect=P(G64, ks=2, fold=9)),
    conv("win_xoff2", 24, 7, 40, B=1, window=(70, 3), x_off=2, x_gap=1, y_gap=2, expect=P(G64, ks=2)),
    conv("win_xoff3", 24, 7, 40, B=2, window=(70, 3), x_off=3, x_gap=2, elu_in=1, expect=P(G64, ks=2)),
    conv("win_dil", 24, 3, 40, B=2, window=(70, 0), dil=3, elu_in=1, expect=P(G64)),
    # residual block's second conv: k = 1, the residual read at offset P of the block's input window
    conv("k1_resid", 20, 1, 40, B=2, window=(70, 2), resid=1, r_off=6, r_gap=1, expect=P(G64)),
    conv("k1_resid_fold", 130, 1, 40, B=3, window=(6, 2), resid=1, r_off=2, elu_out=1, expect=P(G64, ks=2, fold=6)),
    conv("k1_long", 8, 1, 40, B=3, Tin=8200, resid=1, y2=1, expect=P(G64)),           # 1-tap: never the wide tile
    # wide tiles (>= 256 columns, >= 192 wide blocks)
    conv("wide32", 8, 3, 1, B=3, Tin=8200, elu_in=0, expect=P(WIDE, bm=32)),          # the final decoder conv's form
    conv("wide64", 8, 3, 40, B=3, Tin=8200, y2=1, expect=P(WIDE, bm=64)),
    conv("wide128", 8, 3, 130, B=2, Tin=6150, elu_out=1, expect=P(WIDE, bm=128)),
    conv("wide64_k147", 21, 7, 40, B=3, window=(8200, 1), elu_in=1, x_off=1, x_gap=2, expect=P(WIDE, bm=64)),
]


def conv_arrays(c, seed=0):
    rng = np.random.default_rng([seed, c["Cin"], c["k"], c["Cout"], c["Tout"]])
    B, Cin, Cout, k = c["B"], c["Cin"], c["Cout"], c["k"]
    x = acts(rng, B * c["x_bstride"] + 7)
    w = (rng.standard_normal((Cout, Cin * k)) / math.sqrt(Cin * k)).astype(np.float32)
    bias = rng.standard_normal(Cout).astype(np.float32) * np.float32(0.5) if c["bias"] else None
    resid = acts(rng, B * c["r_bstride"] + 3) if c["resid"] else None
    return x, w, bias, resid


def conv_index(c):
    """(x gather index (B, Tout, Cin, k), its validity, y index (B, Tout, Cout), resid index)."""
    B, Cin, Cout, k, Tout, Tin = c["B"], c["Cin"], c["Cout"], c["k"], c["Tout"], c["Tin"]
    u = np.arange(Tout)[:, None] * c["stride"] + np.arange(k)[None, :] * c["dil"] - c["pad_l"]      # (Tout, k)
    valid = (u >= 0) & (u < Tin)
    uc = np.clip(u, 0, Tin - 1)
    xi = (np.arange(B)[:, None, None, None] * c["x_bstride"] + np.arange(Cin)[None, None, :, None] * c["x_cstride"] +
          c["x_off"] + uc[None, :, None, :])
    b, t, co = np.arange(B)[:, None, None], np.arange(Tout)[None, :, None], np.arange(Cout)[None, None, :]
    yi = b * c["y_bstride"] + co * c["y_cstride"] + c["y_off"] + t
    ri = b * c["r_bstride"] + co * c["r_cstride"] + c["r_off"] + t
    return xi, np.broadcast_to(valid[None, :, None, :], xi.shape), yi, ri


def conv_reference(c, x, w, bias, resid):
    """float64 outputs, S and the left-to-right float32 evaluation, each (B, Tout, Cout), before the output
    activation; the y index."""
    xi, valid, yi, ri = conv_index(c)
    a = x[xi]
    if not c["replicate"]:
        a = np.where(valid, a, np.float32(0))
    a64 = a.astype(F64)
    if c["elu_in"]:
        a64 = elu64(a64)
    B, Tout = a.shape[:2]
    cols = a64.reshape(B, Tout, -1)
    w64 = w.astype(F64)
    y64 = cols @ w64.T
    S = np.abs(cols) @ np.abs(w64).T
    lr = lr_sum(cols.astype(np.float32), w)
    if bias is not None:
        y64, S, lr = y64 + bias.astype(F64), S + np.abs(bias.astype(F64)), (lr + bias).astype(np.float32)
    if resid is not None:
        r = resid[ri]
        y64, S, lr = y64 + r.astype(F64), S + np.abs(r.astype(F64)), (lr + r).astype(np.float32)
    return y64, S, lr, yi


def run_conv(c, x, w, bias, resid):
    _lib, L = _L()
    geo = _i32([c[f] for f in CONV_GEO])
    ybuf = np.full(c["B"] * c["y_bstride"] + 11, SENT, np.float32)
    y2buf = ybuf.copy() if c["y2"] else None
    _lib.check(L.mimi_lab_conv1d(_p(geo), len(geo), _p(x), x.size, _p(w), w.size, _p(bias), _p(resid),
                                 0 if resid is None else resid.size, _p(ybuf), _p(y2buf), ybuf.size))
    return ybuf, y2buf


@pytest.mark.parametrize("c", CONV_CASES, ids=[c["name"] for c in CONV_CASES])
def test_conv1d(c):
    assert plan(0, [c[f] for f in CONV_GEO]) == c["expect"]
    x, w, bias, resid = conv_arrays(c)
    y64, S, lr, yi = conv_reference(c, x, w, bias, resid)
    ybuf, y2buf = run_conv(c, x, w, bias, resid)
    post = elu64 if c["elu_out"] else (lambda v: np.asarray(v, F64))
    check(c["name"] + " y", ybuf[yi], post(y64), S, post(lr).astype(np.float32))
    sentinel_intact(ybuf, yi, c["name"] + " y")
    if c["y2"]:
        check(c["name"] + " y2", y2buf[yi], elu64(y64), S, elu64(lr).astype(np.float32))
        sentinel_intact(y2buf, yi, c["name"] + " y2")
        if c["elu_out"] == 0:   # ELU(v) of the stored v is what a consumer would compute: bit-identical
            assert np.array_equal(y2buf[yi] > 0, ybuf[yi] > 0)
            assert np.array_equal(y2buf[yi][ybuf[yi] > 0], ybuf[yi][ybuf[yi] > 0])


# ----------------------------------------------------------------------------- transposed conv
CT_GEO = ("Cin", "Tin", "x_bstride", "x_cstride", "x_off", "Cout", "s", "elu_in", "t_in0", "n_in", "y_bstride",
          "y_cstride", "y_off", "B")


def convtr(name, Cin, Cout, s, t_in0, n_in, B, elu_in=1, bias=1, x_off=0, y_off=0, expect=None):
    Tin = t_in0 + n_in
    x_cs, y_cs = x_off + Tin + (x_off > 0), y_off + n_in * s
    return dict(name=name, op=1, Cin=Cin, Tin=Tin, x_bstride=Cin * x_cs, x_cstride=x_cs, x_off=x_off, Cout=Cout, s=s,
                elu_in=elu_in, t_in0=t_in0, n_in=n_in, y_bstride=Cout * y_cs + 2, y_cstride=y_cs, y_off=y_off, B=B,
                bias=bias, expect=expect)


def _ct_cases():
    out = []
    for s in (4, 5, 6, 8):
        for t0 in (0, 1):
            for n_in in (2, 67):
                for B in (1, 3):
                    # n_in 2: K = 200 (no multiple of 16), split; n_in 67: K = 80, two column tiles
                    Cin = 100 if n_in == 2 else 40
                    fold = n_in if (B > 1 and n_in < 64) else 0
                    ks = {2: 2, 67: 1}[n_in]
                    out.append(convtr(f"s{s}_t{t0}_n{n_in}_b{B}", Cin, 37 + s, s, t0, n_in, B, x_off=t0 * (s % 4),
                                      y_off=(s + n_in) % 3, elu_in=(s + B) % 2, expect=P(G64, ks=ks, fold=fold)))
    out.append(convtr("wide128", 8, 130, 8, 1, 260, 4, expect=P(WIDE, bm=128)))
    out.append(convtr("wide64", 8, 40, 4, 1, 257, 16, expect=P(WIDE, bm=64)))
    return out


CT_CASES = _ct_cases()


def convtr_run_and_reference(c, seed=0):
    _lib, L = _L()
    rng = np.random.default_rng([seed, c["Cin"], c["Cout"], c["s"], c["n_in"], c["B"]])
    B, Cin, Cout, s, n_in, t0 = c["B"], c["Cin"], c["Cout"], c["s"], c["n_in"], c["t_in0"]
    x = acts(rng, B * c["x_bstride"] + 5)
    wt = (rng.standard_normal((s, Cout, Cin * 2)) / math.sqrt(2 * Cin)).astype(np.float32)
    bias = rng.standard_normal(Cout).astype(np.float32) * np.float32(0.5) if c["bias"] else None
    ti = t0 + np.arange(n_in)[:, None] - np.arange(2)[None, :]                                        # (n_in, e)
    xi = (np.arange(B)[:, None, None, None] * c["x_bstride"] + np.arange(Cin)[None, None, :, None] * c["x_cstride"] +
          c["x_off"] + np.maximum(ti, 0)[None, :, None, :])
    a = np.where(np.broadcast_to((ti >= 0)[None, :, None, :], xi.shape), x[xi], np.float32(0)).astype(F64)
    if c["elu_in"]:
        a = elu64(a)
    cols = a.reshape(B, n_in, Cin * 2)                                                               # kk = ci * 2 + e
    w64 = wt.astype(F64)
    y64 = np.einsum("bik,rok->biro", cols, w64)                                                      # (B, n_in, s, Cout)
    S = np.einsum("bik,rok->biro", np.abs(cols), np.abs(w64))
    lr = lr_sum(cols.astype(np.float32), wt.reshape(s * Cout, -1)).reshape(B, n_in, s, Cout)
    if bias is not None:
        y64, S, lr = y64 + bias.astype(F64), S + np.abs(bias.astype(F64)), (lr + bias).astype(np.float32)
    b, i, r, co = np.ix_(np.arange(B), np.arange(n_in), np.arange(s), np.arange(Cout))
    yi = b * c["y_bstride"] + co * c["y_cstride"] + c["y_off"] + i * s + r
    geo = _i32([c[f] for f in CT_GEO])
    ybuf = np.full(B * c["y_bstride"] + 9, SENT, np.float32)
    _lib.check(L.mimi_lab_convtr(_p(geo), len(geo), _p(x), x.size, _p(wt), wt.size, _p(bias), _p(ybuf), ybuf.size))
    return dict(x=x, wt=wt, bias=bias, ybuf=ybuf, yi=yi, y64=y64, S=S, lr=lr)


@pytest.mark.parametrize("c", CT_CASES, ids=[c["name"] for c in CT_CASES])
def test_convtr(c):
    assert plan(1, [c[f] for f in CT_GEO]) == c["expect"]
    r = convtr_run_and_reference(c)
    check(c["name"], r["ybuf"][r["yi"]], r["y64"], r["S"], r["lr"])
    sentinel_intact(r["ybuf"], r["yi"], c["name"])


# ----------------------------------------------------------------------------- linear
LN_GEO = ("M", "K", "xs", "N", "os", "epi", "gelu_erf", "conv_T", "conv_bstride", "accumulate")
STORE, ADD, GELU = 0, 1, 4


def lin(name, M, N, K, epi=STORE, scale=0, gelu_erf=0, conv_T=0, accumulate=0, xs=None, os_=None, expect=None):
    return dict(name=name, op=2, M=M, K=K, xs=K if xs is None else xs, N=N, os=N if os_ is None else os_, epi=epi,
                gelu_erf=gelu_erf, conv_T=conv_T, conv_bstride=N * conv_T + 3 if conv_T else 0, accumulate=accumulate,
                scale=scale, expect=expect)


def _lin_cases():
    out = []
    # split-K of the tiled path by (N, K) and rows (64 x 64 tiles; slices double to <= 512 blocks, >= 64 of K each)
    ks = {(32, 128): {17: 2, 64: 2, 65: 2, 130: 2}, (512, 2048): {17: 32, 64: 32, 65: 32, 130: 16},
          (12, 128): {1: 2, 16: 2, 17: 2, 64: 2, 65: 2, 130: 2}, (128, 40): {17: 1, 64: 1, 65: 1, 130: 1}}
    epis = [dict(epi=STORE), dict(epi=ADD, scale=1), dict(epi=ADD), dict(epi=GELU), dict(epi=GELU, gelu_erf=1)]
    i = 0
    for (N, K) in ((32, 128), (512, 2048), (12, 128), (128, 40)):
        for M in (1, 16, 17, 64, 65, 130):
            e = epis[i % len(epis)]
            i += 1
            gemv = M <= 16 and N % 8 == 0        # (12, 128) leaves the GEMV at <= 16 rows
            exp = P(GEMV) if gemv else P(G64, ks=ks[(N, K)][M])
            tag = {STORE: "store", ADD: "add", GELU: "gelu"}[e["epi"]] + ("_scale" if e.get("scale") else "") + \
                ("_erf" if e.get("gelu_erf") else "")
            out.append(lin(f"m{M}_n{N}_k{K}_{tag}", M, N, K, expect=exp, **e))
    # every epilogue on both paths at one shape each, erf GELU on the tiled path with a K tail
    for e in epis:
        tag = {STORE: "store", ADD: "add", GELU: "gelu"}[e["epi"]] + ("_scale" if e.get("scale") else "") + \
            ("_erf" if e.get("gelu_erf") else "")
        out.append(lin(f"gemv_m3_{tag}", 3, 64, 128, expect=P(GEMV), **e))
        out.append(lin(f"tile_m70_{tag}", 70, 72, 200, xs=208, os_=75, expect=P(G64, ks=2), **e))
    for acc in (0, 1):
        # (712 features: 2,136 outputs.  At 72 -- 216 outputs -- the largest of so few rounding errors is too noisy a
        # statistic for a 1.5 x bar: the accumulating store sat at 1.3 x it, at an error of 1.6e-7 S, 1.3 ulp of S)
        out.append(lin(f"convT_acc{acc}_m3", 3, 712, 40, conv_T=3, accumulate=acc, expect=P(G64)))
        out.append(lin(f"convT_acc{acc}_m70", 70, 72, 256, conv_T=35, accumulate=acc, expect=P(G64, ks=4)))
    out.append(lin("wide128", 300, 8200, 24, expect=P(WIDE, bm=128)))   # activation rows are the tile's columns
    return out


LIN_CASES = _lin_cases()


@pytest.mark.parametrize("c", LIN_CASES, ids=[c["name"] for c in LIN_CASES])
def test_linear(c):
    _lib, L = _L()
    assert plan(2, [c[f] for f in LN_GEO]) == c["expect"]
    M, N, K = c["M"], c["N"], c["K"]
    rng = np.random.default_rng([2, M, N, K, c["epi"]])
    x = acts(rng, (M - 1) * c["xs"] + K + 2)
    W = (rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32)
    scale = (rng.standard_normal(N) * 0.5).astype(np.float32) if c["scale"] else None
    xm = np.lib.stride_tricks.as_strided(x, (M, K), (c["xs"] * 4, 4))
    x64, W64 = xm.astype(F64), W.astype(F64)
    y64, S = x64 @ W64.T, np.abs(x64) @ np.abs(W64).T
    lr = lr_sum(xm, W)
    if c["conv_T"]:
        T = c["conv_T"]
        m, n = np.arange(M)[:, None], np.arange(N)[None, :]
        oi = (m // T) * c["conv_bstride"] + n * T + m % T
        size = (M // T) * c["conv_bstride"] + 5
    else:
        oi = np.arange(M)[:, None] * c["os"] + np.arange(N)[None, :]
        size = (M - 1) * c["os"] + N + 6
    init = np.full(size, SENT, np.float32)
    post = lambda v: np.asarray(v, F64)                                                         # noqa: E731
    if c["epi"] == ADD or c["accumulate"]:
        old = acts(rng, (M, N))
        init[oi] = old
        sc = scale if (scale is not None and not c["conv_T"]) else np.ones(N, np.float32)
        y64, S = old.astype(F64) + sc.astype(F64) * y64, np.abs(old.astype(F64)) + np.abs(sc.astype(F64)) * S
        lr = (old + (sc * lr).astype(np.float32)).astype(np.float32)
    elif c["epi"] == GELU and not c["conv_T"]:
        post = lambda v: gelu64(v, c["gelu_erf"])                                                # noqa: E731
    geo = _i32([c[f] for f in LN_GEO])
    out = init.copy()
    _lib.check(L.mimi_lab_linear(_p(geo), len(geo), _p(x), x.size, _p(W), W.size, _p(scale), _p(out), out.size))
    check(c["name"], out[oi], post(y64), S, post(lr).astype(np.float32))
    mask = np.ones(out.shape, bool)
    mask[oi.reshape(-1)] = False
    assert np.array_equal(out[mask].view(np.uint32), init[mask].view(np.uint32)), "a store outside the addressed region"


# ----------------------------------------------------------------------------- LayerNorm rows
LN_ROWS, LN_EPS = 300, 1e-5
LN_CASES = [(D, M) for D in (32, 40, 256, 512) for M in (1, 63, LN_ROWS)]


def _ln_data(D):
    """LN_ROWS rows of three classes (the kernel runs the first M of them), weights and biases some negative:
    "far": mean 100, std 0.01 (a one-pass E[x^2] - E[x]^2 variance would lose them); "flat": all elements 1.5
    (variance 0: eps alone; every partial sum of 1.5 is exact in float32, so the mean is too); "plain": the rest."""
    rng = np.random.default_rng([4, D])
    x = acts(rng, (LN_ROWS, D)) * rng.uniform(0.1, 4.0, (LN_ROWS, 1)).astype(np.float32)
    cls = np.array(["plain"] * LN_ROWS, object)
    cls[3::4], cls[[7, 200]] = "far", "flat"
    far = cls == "far"
    x[far] = (100.0 + 0.01 * rng.standard_normal((int(far.sum()), D))).astype(np.float32)
    x[cls == "flat"] = np.float32(1.5)
    w = (rng.standard_normal(D) * 0.8).astype(np.float32)
    b = (rng.standard_normal(D) * 0.5).astype(np.float32)
    assert (w < 0).any() and (b < 0).any()
    return x, w, b, cls


def _ln_two_pass(x, w, b, dt):
    x, w, b = x.astype(dt), w.astype(dt), b.astype(dt)
    mean = x.sum(-1, keepdims=True, dtype=dt) / dt(x.shape[-1])
    c = x - mean
    var = (c * c).sum(-1, keepdims=True, dtype=dt) / dt(x.shape[-1])
    return c * (dt(1) / np.sqrt(var + dt(LN_EPS))) * w + b


def _ln_err(y, y64):
    """Per row: max |y - float64| / the row's largest |float64 value|."""
    return np.abs(np.asarray(y, F64) - y64).max(-1) / np.abs(y64).max(-1)


@pytest.mark.parametrize("D,M", LN_CASES, ids=[f"d{D}_m{M}" for D, M in LN_CASES])
def test_layernorm(D, M):
    """layernorm_rows_kernel through mimi_lab_layernorm against a float64 LayerNorm.  D = 32 and 40 leave most of
    the block's 256 threads without an element, 256 gives each one, 512 two; M = 1, 63, 300 rows (one block a row).
    Unit: per row, max |got - float64| / the row's largest |float64 value|.  Bar, as test_linear's: 1.5 x the error of
    a plain float32 two-pass evaluation in numpy (mean, centred squares, one rsqrt) in that unit, measured each run --
    the margin is ``check``'s, this file's for every element-wise case.  The bar is taken per row class over all
    LN_ROWS rows of the class the case's rows are drawn from (the largest of one row's D rounding errors is too
    noisy a statistic for a 1.5 x bar, cf. LIN_CASES' convT note), and a class is held to its own bar: the "far"
    rows' float32 error is that of a mean rounded at 100 against a spread of 0.01, about 1e4 x the others'.
    A "flat" row must come out as the bias exactly.  Stores past M x D must not happen."""
    _lib, L = _L()
    x, w, b, cls = _ln_data(D)
    y64 = _ln_two_pass(x, w, b, F64)
    e32 = _ln_err(_ln_two_pass(x, w, b, np.float32), y64)
    out = np.full(M * D + 7, SENT, np.float32)
    xin = np.ascontiguousarray(x[:M])
    _lib.check(L.mimi_lab_layernorm(M, D, _p(xin), _p(w), _p(b), LN_EPS, _p(out), out.size))
    assert (out[M * D:].view(np.uint32) == SENT.view(np.uint32)).all(), "a store outside the addressed region"
    got = out[:M * D].reshape(M, D)
    err = _ln_err(got, y64[:M])
    for c in ("plain", "far"):
        rows = np.flatnonzero(cls[:M] == c)
        if not rows.size:
            continue
        bar = 1.5 * float(e32[cls == c].max())
        worst = float(err[rows].max())
        print(f"layernorm d{D}_m{M} {c}: err {worst:.3e} bar {bar:.3e} ratio {worst / bar:.2f}")
        assert bar > 0
        assert worst <= bar, f"{c}: {worst:.3e} > {bar:.3e} at row {int(rows[err[rows].argmax()])}"
    for r in np.flatnonzero(cls[:M] == "flat"):
        assert np.array_equal(got[r].view(np.uint32), b.view(np.uint32)), f"flat row {r}: (x - mean) is not 0"
    with pytest.raises(ValueError):
        _lib.check(L.mimi_lab_layernorm(M, D, _p(xin), _p(w), _p(b), LN_EPS, _p(out), M * D - 1))


# ----------------------------------------------------------------------------- RVQ encode
def _rvq_data(cd, M, seed, dup=False):
    rng = np.random.default_rng([3, cd, M, seed])
    bins, n_q = 512, 3
    cb = rng.standard_normal((n_q, bins, cd)).astype(np.float32)
    if dup:
        cb[0, 300], cb[0, 11] = cb[0, 3], cb[0, 10]
    # |c|^2 / 2 summed in float64, rounded once (the engine's finish_codebook)
    c2 = ((cb.astype(F64) ** 2).sum(-1) / 2).astype(np.float32)
    r = (rng.standard_normal((M, cd)) * 1.5).astype(np.float32)
    if dup:
        r[0::4], r[1::4] = cb[0, 300], cb[0, 11]
    return cb, c2, r


def _rvq_run(gemm, cb, c2, r, T):
    _lib, L = _L()
    n_q, bins, cd = cb.shape
    M = r.shape[0]
    res, codes = r.copy(), np.full((M // T, n_q, T), -5, np.int32)
    _lib.check(L.mimi_lab_rvq_encode(gemm, M, T, cd, bins, n_q, 0, n_q, _p(cb), _p(c2), _p(res), _p(codes)))
    return codes, res


@pytest.mark.parametrize("cd", [32, 256])
@pytest.mark.parametrize("M", [1, 63, 64, 300])
@pytest.mark.parametrize("dup", [False, True], ids=["normal", "first_min"])
def test_rvq_encode(cd, M, dup):
    """Rows 1 and 63 on the per-row kernel as the codec would run them, 64 and 300 (ragged last row tile) on
    the distance GEMM; both kernels run on every case's data and must agree bit for bit (their documented
    contract).  Against float64: every chosen code's float64 distance lies within 2 x (the left-to-right float32
    error of that row's dots) of the float64 minimum -- no frame excluded.  first_min: the codebook has exact
    duplicate rows (3, 300) and (10, 11) and input rows equal to them: both kernels return the lower index."""
    cb, c2, r = _rvq_data(cd, M, 0, dup)
    T = M if M < 64 else M // 4 if M % 4 == 0 else M
    (codes_a, res_a), (codes_b, res_b) = _rvq_run(0, cb, c2, r, T), _rvq_run(1, cb, c2, r, T)
    assert np.array_equal(codes_a, codes_b), np.argwhere(codes_a != codes_b)[:4].tolist()
    assert np.array_equal(res_a.view(np.uint32), res_b.view(np.uint32))
    n_q, bins, _ = cb.shape
    got = codes_a.transpose(0, 2, 1).reshape(M, n_q)                          # codes [b][k][t], row m = b * T + t
    assert got.min() >= 0 and got.max() < bins
    if dup:
        assert (got[0::4, 0] == 3).all() and (got[1::4, 0] == 10).all(), (got[0::4, 0], got[1::4, 0])
    res = r.copy()
    for k in range(n_q):
        d64 = c2[k].astype(F64)[None, :] - res.astype(F64) @ cb[k].astype(F64).T                   # (M, bins)
        e_lr = np.abs(lr_sum(res, cb[k]).astype(F64) - res.astype(F64) @ cb[k].astype(F64).T).max(-1)
        chosen = np.take_along_axis(d64, got[:, k: k + 1].astype(np.int64), -1)[:, 0]
        over = (chosen - d64.min(-1)) - 2 * e_lr
        assert (over <= 0).all(), f"codebook {k}: row {int(over.argmax())} chose a code {over.max():.3e} past the bar"
        res = (res - cb[k][got[:, k]]).astype(np.float32)                    # one rounding per element, as the kernels
    assert np.array_equal(res.view(np.uint32), res_a.view(np.uint32)), "final residual"


# ----------------------------------------------------------------------------- fold and batch
FOLD_CONV = ["win_n2_b3", "win_n6_b11", "down_b3", "k1_resid_fold", "win_xoff3"]
FOLD_CT = ["s4_t1_n2_b3", "s5_t0_n2_b3", "s8_t1_n67_b3"]


@pytest.mark.parametrize("name", FOLD_CONV)
def test_conv1d_batched_equals_single(name):
    """Folding leaves every output's summation order unchanged: a batched call and each utterance alone are
    bit-identical wherever both split K alike (elsewhere test_conv1d's float64 bar holds both)."""
    c = next(c for c in CONV_CASES if c["name"] == name)
    x, w, bias, resid = conv_arrays(c)
    ybuf, _ = run_conv(c, x, w, bias, resid)
    _, _, yi, _ = conv_index(c)
    one = dict(c, B=1, y2=0)
    same = plan(0, [one[f] for f in CONV_GEO])["ks"] == c["expect"]["ks"]
    y64, S, lr, _ = conv_reference(c, x, w, bias, resid)
    post = elu64 if c["elu_out"] else (lambda v: np.asarray(v, F64))
    for b in range(c["B"]):
        xb = np.ascontiguousarray(x[b * c["x_bstride"]:])
        rb = None if resid is None else np.ascontiguousarray(resid[b * c["r_bstride"]:])
        yb, _ = run_conv(one, xb, w, bias, rb)
        alone = yb[yi[0]]
        if same:
            assert np.array_equal(alone.view(np.uint32), ybuf[yi[b]].view(np.uint32)), f"utterance {b}"
        else:
            check(f"{name} alone {b}", alone, post(y64[b]), S[b], post(lr[b]).astype(np.float32))


@pytest.mark.parametrize("name", FOLD_CT)
def test_convtr_batched_equals_single(name):
    _lib, L = _L()
    c = next(c for c in CT_CASES if c["name"] == name)
    r = convtr_run_and_reference(c)
    one = dict(c, B=1)
    same = plan(1, [one[f] for f in CT_GEO])["ks"] == c["expect"]["ks"]
    geo = _i32([one[f] for f in CT_GEO])
    for b in range(c["B"]):
        xb = np.ascontiguousarray(r["x"][b * c["x_bstride"]:])
        yb = np.full(c["y_bstride"] + 9, SENT, np.float32)
        _lib.check(L.mimi_lab_convtr(_p(geo), len(geo), _p(xb), xb.size, _p(r["wt"]), r["wt"].size, _p(r["bias"]), _p(yb),
                                     yb.size))
        alone = yb[r["yi"][0]]
        if same:
            assert np.array_equal(alone.view(np.uint32), r["ybuf"][r["yi"][b]].view(np.uint32)), f"utterance {b}"
        else:
            check(f"{name} alone {b}", alone, r["y64"][b], r["S"][b], r["lr"][b])


# ----------------------------------------------------------------------------- bad input, coverage
def test_bad_geometry_is_refused():
    """A geometry that does not fit its arrays is CSM_ERR_ARG (ValueError) before anything is launched."""
    _lib, L = _L()
    c = CONV_CASES[0]
    x, w, bias, resid = conv_arrays(c)
    geo = _i32([c[f] for f in CONV_GEO])
    ybuf = np.full(c["B"] * c["y_bstride"] + 11, SENT, np.float32)
    for bad in (dict(x_n=x.size - 60), dict(y_n=5), dict(w_n=w.size - 1), dict(n_geo=20)):
        rc = L.mimi_lab_conv1d(_p(geo), bad.get("n_geo", len(geo)), _p(x), bad.get("x_n", x.size), _p(w),
                               bad.get("w_n", w.size), _p(bias), None, 0, _p(ybuf), None, bad.get("y_n", ybuf.size))
        assert rc == _lib.CSM_ERR_ARG, bad
    for field, v in (("Cin", 0), ("stride", 0), ("x_off", -1), ("y_cstride", -4), ("B", 0), ("Tout", -1)):
        g = _i32([v if f == field else c[f] for f in CONV_GEO])
        assert L.mimi_lab_plan(0, _p(g), len(g), _p(np.zeros(4, np.int32))) == _lib.CSM_ERR_ARG, field
    assert (ybuf.view(np.uint32) == SENT.view(np.uint32)).all()
    ct = CT_CASES[0]
    g = _i32([ct["Tin"] + 5 if f == "n_in" else ct[f] for f in CT_GEO])
    assert L.mimi_lab_plan(1, _p(g), len(g), _p(np.zeros(4, np.int32))) == _lib.CSM_ERR_ARG
    ln = LIN_CASES[0]
    g = _i32([ln["K"] - 1 if f == "xs" else ln[f] for f in LN_GEO])
    assert L.mimi_lab_plan(2, _p(g), len(g), _p(np.zeros(4, np.int32))) == _lib.CSM_ERR_ARG
    cb, c2, r = _rvq_data(32, 4, 0)
    codes = np.zeros((1, 3, 4), np.int32)
    assert L.mimi_lab_rvq_encode(1, 4, 4, 30, 512, 3, 0, 3, _p(cb), _p(c2), _p(r), _p(codes)) == _lib.CSM_ERR_ARG
    assert L.mimi_lab_rvq_encode(0, 4, 3, 32, 512, 3, 0, 3, _p(cb), _p(c2), _p(r), _p(codes)) == _lib.CSM_ERR_ARG


def test_table_reaches_every_branch():
    """The plans the cases above assert, taken together: every kernel kind, every split factor, fold on and
    off, split launches whose K is no multiple of 16 -- so a later retune of a threshold cannot silently
    empty a branch (the per-case plan asserts then fail first; this one says what is no longer reached)."""
    cases = CONV_CASES + CT_CASES + LIN_CASES
    plans = [c["expect"] for c in cases]
    kinds = {(p["kernel"], p["bm"]) for p in plans}
    assert kinds >= {(GEMV, 0), (G64, 0), (WIDE, 32), (WIDE, 64), (WIDE, 128)}, kinds
    assert {p["ks"] for p in plans} >= {1, 2, 4, 8, 16, 32}
    for op in (0, 1):
        assert {bool(p["fold"]) for c, p in zip(cases, plans) if c["op"] == op} == {False, True}

    def kdim(c):
        return c["Cin"] * c["k"] if c["op"] == 0 else c["Cin"] * 2 if c["op"] == 1 else c["K"]
    for op in (0, 1, 2):
        assert any(c["op"] == op and p["ks"] > 1 and kdim(c) % 16 for c, p in zip(cases, plans)), op
    # (no wide launch splits: tests/test_abi_cpu.py::test_mimi_wide_plan_never_splits sweeps the plan's thresholds)
    assert {c["op"] for c, p in zip(cases, plans) if p["kernel"] == WIDE} == {0, 1, 2}
