"""csrc/lm.hip and unispeech_amd/transformer_lm.py on the device.  Reads tests/golden/ only.

Kernel wavlm_lm_logprob: against float64 on the same bf16-valued inputs (so the operands are exact in both dtypes); bound
F32_TOL = 5e-5 of max(max |z|, max |logprob|), the project's fp32-kernel bound (tests/test_diarization_gpu.py).  Kernel
wavlm_attn_causal_fwd: against the float64 causal softmax, that file's kernel_tol(dtype) of |V|'s maximum.  Model: fp32 mode
within HEAD_TOL = 5e-4 of the fixture's largest magnitude, bf16 mode within 2 * e_ref (the reference itself in bf16 on the CPU).
Rescoring: every s2 within rescore_weight * (words + 1) * tol_token of rescore_reference, and the same winner.

At production geometry (tests/transformer_lm_cases.py holds the built cases, tests/test_transformer_lm.py what they rest on): the
output layer at D 1024 with 16 K stages per tile, four slabs and three row blocks; D = 8 (mod 16) with NaN behind D in both
operands; the slab and row-block edges; V 200 003; a target in every accumulator slot; logits that rise tile by tile (the
rescaling of the running sum); the attention at T 300 over lengths on and around the 64- and 128-key edges, 0 included, with
scores that rise step by step; B * H 65 520; and models W and X of tests/golden/transformer_lm_wide.npz."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import transformer_lm_cases as C
from conftest import load_golden

pytestmark = pytest.mark.gpu

F32_TOL, BF16_TOL, HEAD_TOL = 5e-5, 2.0 ** -8, 5e-4
DTYPES = [torch.float32, torch.bfloat16]


def kernel_tol(dtype):
    return F32_TOL + (BF16_TOL if dtype == torch.bfloat16 else 0.0)


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_memory_behind():
    import gc
    from unispeech_amd import ops
    saved = dict(ops._WS)
    yield
    torch.cuda.synchronize()
    ops._WS.clear()
    ops._WS.update(saved)
    C.rescoring.cache_clear()
    for cached in (logprob_case, long_causal_ref, C.slot_case, C.staircase_case):
        cached.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------- wavlm_lm_logprob
@functools.lru_cache(maxsize=None)
def logprob_case(R, V, D, scale=1.0):
    """bf16-valued X [R, D], W [V, D] (fp32 tensors), targets with the special columns, and the float64 results; computed once
    per shape and never written to"""
    g = torch.Generator().manual_seed(1000 * R + 10 * V + D)
    X = (torch.randn(R, D, generator=g).to(torch.bfloat16).float() * scale)
    W = torch.randn(V, D, generator=g).to(torch.bfloat16).float()
    tgt = torch.randint(0, V, (R,), generator=g, dtype=torch.int32)
    special = [0, V - 1, min(127, V - 1), min(128, V - 1), min(2047, V - 1), min(2048, V - 1), -1, V, -7, V + 1000]
    for r, t in enumerate(special):            # column 0, V - 1, both sides of a tile and of a slab boundary, negative, >= V
        if r + 1 < R:
            tgt[r + 1] = t
    if R == 1:
        tgt[0] = V - 1
    z = X.double().numpy() @ W.double().numpy().T
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    t = tgt.numpy()
    ok = (t >= 0) & (t < V)
    lp = np.where(ok, z[np.arange(R), np.clip(t, 0, V - 1)] - lse, np.where(t < 0, 0.0, np.nan))
    return X, W, tgt, z, lse, lp


def fp32_cpu_error(case):
    """e32: the same case in plain float32 on the CPU (torch matmul and logsumexp) against float64, logprob and lse"""
    X, W, tgt, z, lse, lp = case
    z32 = X @ W.t()
    lse32 = torch.logsumexp(z32, 1)
    ok = torch.from_numpy(~np.isnan(lp)) & (tgt >= 0)
    lp32 = (z32[torch.arange(X.shape[0]), tgt.long().clamp(0, W.shape[0] - 1)] - lse32).double().numpy()
    return max(np.abs(lp32 - lp)[ok.numpy()].max(), np.abs(lse32.double().numpy() - lse).max())


def check_logprob(got, lse_got, case, what, e32=None):
    """e32 given: the bound is max(F32_TOL * max(max |z|, max |logprob|), 4 * e32) -- 4 for another summation order of the same
    precision"""
    X, W, tgt, z, lse, lp = case
    got = f64(got)
    nan = np.isnan(lp)
    assert np.array_equal(np.isnan(got), nan), what
    assert (got[tgt.numpy() < 0] == 0).all(), what
    bound = F32_TOL * max(np.abs(z).max(), np.abs(lp[~nan]).max())
    if e32 is not None:
        print("%s: bound %.3e, e32 %.3e, 4 e32 %s the bound" % (what, bound, e32, "above" if 4 * e32 > bound else "below"))
        bound = max(bound, 4 * e32)
    err = np.abs(got[~nan] - lp[~nan]).max()
    msg = "%s: logprob error %.3e" % (what, err)
    if lse_got is not None:
        el = np.abs(f64(lse_got) - lse).max()
        msg += ", lse error %.3e" % el
        assert el <= bound, (what, el, bound)
    print(msg, "bound %.3e (max |z| %.1f)" % (bound, np.abs(z).max()))
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [32, 80])
@pytest.mark.parametrize("V", [5, 257, 2051])
@pytest.mark.parametrize("R", [1, 130])
def test_logprob_kernel_against_fp64(R, V, D, dtype):
    from unispeech_amd import ops
    case = logprob_case(R, V, D)
    X, W, tgt = (t.cuda() for t in case[:3])
    lp, lse = ops.lm_logprob(X.to(dtype), W.to(dtype), tgt, want_lse=True)
    assert lp.dtype == lse.dtype == torch.float32 and lp.shape == lse.shape == (R,)
    check_logprob(lp, lse, case, "R %d V %d D %d %s" % (R, V, D, dtype))
    lp2, _ = ops.lm_logprob(X.to(dtype), W.to(dtype), tgt)                       # lse is optional
    assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_logprob_kernel_keeps_a_running_maximum(dtype):
    """|z| reaches about 300: exp overflows fp32 without the running maximum"""
    from unispeech_amd import ops
    case = logprob_case(130, 2051, 80, scale=8.0)
    assert 200 <= np.abs(case[3]).max() <= 450
    X, W, tgt = (t.cuda() for t in case[:3])
    lp, lse = ops.lm_logprob(X.to(dtype), W.to(dtype), tgt, want_lse=True)
    check_logprob(lp, lse, case, "scaled %s" % dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_logprob_rows_are_independent_and_runs_reproducible(dtype):
    from unispeech_amd import ops
    X, W, tgt = (t.cuda() for t in logprob_case(130, 2051, 80)[:3])
    X, W = X.to(dtype), W.to(dtype)
    a, la = ops.lm_logprob(X, W, tgt, want_lse=True)
    b, lb = ops.lm_logprob(X, W, tgt, want_lse=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(la, lb)
    one, lone = ops.lm_logprob(X[77:78].contiguous(), W, tgt[77:78].contiguous(), want_lse=True)
    assert torch.equal(one.view(torch.int32), a[77:78].view(torch.int32)) and torch.equal(lone, la[77:78])
    # a view with a row stride: the same rows out of a wider tensor
    wide = torch.zeros(130, 96, dtype=dtype, device="cuda")
    wide[:, :80] = X
    c, _ = ops.lm_logprob(wide[:, :80], W, tgt)
    assert torch.equal(c.view(torch.int32), a.view(torch.int32))


def strided(t, pad, dtype):
    """t [N, D] as the first D columns of a [N, D + pad] device tensor whose other columns hold NaN"""
    wide = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=dtype, device="cuda")
    wide[:, :t.shape[1]] = t.to(dtype)
    return wide[:, :t.shape[1]]


LOGPROB_SHAPES = {                                      # name: (R, V, D, columns of NaN behind D in X and in W)
    "production-width": (300, 6200, 1024, 0),           # 16 K stages per tile, 4 slabs (the last: 56 entries), 3 row blocks (44 rows)
    "ragged-k-8": (130, 2051, 8, 8),                    # D = 8 (mod 16): the last MFMA step is half zero fill
    "ragged-k-24": (130, 2051, 24, 8),
    "ragged-k-200": (130, 2051, 200, 8),                # 4 K stages, the last one 8 wide
    "slab-2048": (130, 2048, 80, 0),
    "slab-2049": (130, 2049, 80, 0),
    "slab-4096": (130, 4096, 80, 0),
    "slab-2048+128+1": (130, 2048 + 128 + 1, 80, 0),    # a last slab with a full tile and a partial one
    "large-vocabulary": (5, 200003, 16, 0),             # 98 slabs
    "rows-127": (127, 257, 32, 0),
    "rows-128": (128, 257, 32, 0),
    "rows-129": (129, 257, 32, 0),
    "rows-257": (257, 257, 32, 0),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(LOGPROB_SHAPES))
def test_logprob_kernel_at_production_geometry(shape, dtype):
    """logprob and lse against float64.  At D 1024 the bound is max(F32_TOL * max(max |z|, max |logprob|), 4 * e32), e32 being
    plain float32 on the CPU against float64; both are printed (DESIGN.md 4.12 records them)."""
    from unispeech_amd import ops
    R, V, D, pad = LOGPROB_SHAPES[shape]
    case = logprob_case(R, V, D)
    X, W = strided(case[0], pad, dtype), strided(case[1], pad, dtype)
    assert X.stride(0) == W.stride(0) == D + pad
    lp, lse = ops.lm_logprob(X, W, case[2].cuda(), want_lse=True)
    check_logprob(lp, lse, case, "%s R %d V %d D %d %s" % (shape, R, V, D, dtype), fp32_cpu_error(case) if D >= 1024 else None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_logprob_target_in_every_accumulator_slot(dtype):
    """R 256, V 2051, D 32: each block of 128 rows has a target at every position of a tile (tests/test_transformer_lm.py)"""
    from unispeech_amd import ops
    case = C.slot_case()
    X, W, tgt = (t.cuda() for t in case[:3])
    lp, lse = ops.lm_logprob(X.to(dtype), W.to(dtype), tgt, want_lse=True)
    check_logprob(lp, lse, case, "slots %s" % dtype)
    # the target's logit alone, so that an error of lse cannot hide one of the gather
    tz = f64(lp) + f64(lse)
    want = case[3][np.arange(256), tgt.cpu().numpy()]
    assert np.abs(tz - want).max() <= 2 * F32_TOL * np.abs(case[3]).max()


@pytest.mark.parametrize("dtype", DTYPES)
def test_logprob_rescales_the_running_sum(dtype):
    """the staircase: the running maximum is renewed at nearly every tile and every slab carries weight, so a kernel that drops
    or misapplies exp(m_old - m_new), over tiles or over slabs, is off by far more than the bound (2.7 in lse on the c = 2 row)"""
    from unispeech_amd import ops
    case = C.staircase_case()
    X, W, tgt = (t.cuda() for t in case[:3])
    lp, lse = ops.lm_logprob(X.to(dtype), W.to(dtype), tgt, want_lse=True)
    check_logprob(lp, lse, case, "staircase %s" % dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_logprob_bitwise_claims_at_production_width(dtype):
    """(300, 6200, 1024): two runs agree; row 299 alone equals its bits in the batch; W as the first D columns of a wider table
    gives the bits of a contiguous W"""
    from unispeech_amd import ops
    R, V, D = 300, 6200, 1024
    X, W, tgt = (t.cuda() for t in logprob_case(R, V, D)[:3])
    X, W = X.to(dtype), W.to(dtype)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    a, la = ops.lm_logprob(X, W, tgt, want_lse=True)
    b, lb = ops.lm_logprob(X, W, tgt, want_lse=True)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(la), bits(lb))
    one, lone = ops.lm_logprob(X[299:300].contiguous(), W, tgt[299:300].contiguous(), want_lse=True)
    assert torch.equal(bits(one), bits(a[299:300])) and torch.equal(bits(lone), bits(la[299:300]))
    table = strided(W, 64, dtype)
    assert table.stride(0) == D + 64
    c, lc = ops.lm_logprob(X, table, tgt, want_lse=True)
    assert torch.equal(bits(c), bits(a)) and torch.equal(bits(lc), bits(la))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,V,D", [(130, 2051, 80), (130, 257, 32), (1, 5, 32)])
def test_composed_switch_agrees(monkeypatch, R, V, D, dtype):
    """WAVLM_LM_LOGPROB_COMPOSED=1: wavlm_gemm into fp32 logits + wavlm_ce_rows; read at every call"""
    from unispeech_amd import ops, transformer_lm as T
    case = logprob_case(R, V, D)
    X, W, tgt = (t.cuda() for t in case[:3])
    calls = []
    real = ops.lm_logprob
    monkeypatch.setattr(ops, "lm_logprob", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(T, "COMPOSED_BUDGET_BYTES", 64 * 4 * ((V + 3) // 4 * 4))           # several row chunks at R = 130
    monkeypatch.setenv("WAVLM_LM_LOGPROB_COMPOSED", "1")
    lp, lse = T.lm_logprob(X.to(dtype), W.to(dtype), tgt)
    assert not calls and lse is None
    check_logprob(lp, None, case, "composed R %d V %d D %d %s" % (R, V, D, dtype))
    monkeypatch.setenv("WAVLM_LM_LOGPROB_COMPOSED", "0")
    lp2, _ = T.lm_logprob(X.to(dtype), W.to(dtype), tgt)
    assert calls == [1]
    check_logprob(lp2, None, case, "kernel")


def test_logprob_refuses_bad_arguments():
    """-1 before any launch: an unsupported shape, a NULL pointer, a leading dimension below D, a misaligned pointer, a short
    workspace"""
    from unispeech_amd import _lib, ops
    h = _lib.lib()
    R, D, V = 4, 32, 300
    x = torch.zeros(R + 1, D, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(V, D, dtype=torch.bfloat16, device="cuda")
    t = torch.zeros(R, dtype=torch.int32, device="cuda")
    out = torch.zeros(R, device="cuda")
    need = h.wavlm_lm_logprob_workspace_bytes(R, V)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    p = ops.ptr

    def call(X=p(x), ldx=D, Wp=p(w), ldw=D, dt=1, tp=p(t), D_=D, V_=V, o=p(out), wsp=p(ws), nb=need):
        return h.wavlm_lm_logprob(X, ldx, Wp, ldw, dt, tp, R, D_, V_, o, None, wsp, nb, ops.stream())
    assert call() == 0
    assert call(D_=36) == -1 and call(D_=4) == -1 and call(V_=0) == -1 and call(dt=2) == -1
    assert call(X=None) == -1 and call(Wp=None) == -1 and call(tp=None) == -1 and call(o=None) == -1 and call(wsp=None) == -1
    assert call(ldx=D - 8) == -1 and call(ldw=D - 8) == -1 and call(ldx=D + 4) == -1
    assert call(X=ops.ptr(x, 4)) == -1 and call(Wp=ops.ptr(w, 1)) == -1
    assert call(nb=need - 1) == -1
    assert h.wavlm_attn_causal_fwd(p(x), p(w), None, 1, 1, 1, 16, 1, ctypes.c_float(1.0), ops.stream()) == -1
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------- wavlm_attn_causal_fwd
def causal_ref(qkv, H, lengths):
    B, T, D3 = qkv.shape
    d = D3 // (3 * H)
    out = np.zeros((B, T, H * d))
    for b, L in enumerate(lengths):
        if L < 1:                                                                # every row of the sequence is zero
            continue
        q, k, v = (qkv[b, :L, i * H * d:(i + 1) * H * d].reshape(L, H, d).transpose(1, 0, 2) for i in range(3))
        s = q @ k.transpose(0, 2, 1) / np.sqrt(d)
        s = np.where(np.triu(np.ones((L, L), dtype=bool), 1)[None], -np.inf, s)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        out[b, :L] = (p @ v).transpose(1, 0, 2).reshape(L, H * d)
    return out


def causal_case(d, dtype):
    g = torch.Generator().manual_seed(d)
    B, H, T = 3, 2, 130
    qkv = torch.randn(B, T, 3 * H * d, generator=g)
    qkv[..., :H * d] *= 1.5
    qkv[..., 2 * H * d:] += 0.5
    return qkv.to(dtype).cuda(), H, [130, 33, 1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [32, 64])
def test_causal_attention_against_fp64(d, dtype):
    from unispeech_amd import ops
    qkv, H, lengths = causal_case(d, dtype)
    il = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    o = ops.attn_causal_fwd(qkv, H, il)
    want = causal_ref(f64(qkv), H, lengths)
    assert o.shape == (3, 130, H * d) and o.dtype == dtype
    vmax = np.abs(f64(qkv[..., 2 * H * d:])).max()
    err = np.abs(f64(o) - want).max()
    print("causal attention", dtype, d, "error", err, "of |V| max", vmax, "=", err / vmax)
    assert np.isfinite(f64(o)).all() and err <= kernel_tol(dtype) * vmax, (err, vmax)
    for b, L in enumerate(lengths):                                              # rows beyond a length are zero
        assert not f64(o[b, L:]).any()
    # sequence 1 alone at T = 33: bitwise its rows in the batch; and no lengths = every sequence T long
    alone = ops.attn_causal_fwd(qkv[1:2, :33].contiguous(), H, il[1:2].contiguous())
    assert torch.equal(alone[0].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       o[1, :33].view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    full = ops.attn_causal_fwd(qkv, H)
    assert np.abs(f64(full) - causal_ref(f64(qkv), H, [130] * 3)).max() <= kernel_tol(dtype) * vmax
    assert torch.equal(full[0], o[0])
    # the row of a padded position may hold anything: the result must not read it
    poisoned = qkv.clone()
    poisoned[1, 33:] = float("nan")
    poisoned[2, 1:] = float("inf")
    assert torch.equal(ops.attn_causal_fwd(poisoned, H, il), o)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@functools.lru_cache(maxsize=None)
def long_causal_ref(d):
    """the long case's float64 result and max |V|: bf16-valued inputs, so one reference serves both dtypes"""
    qkv = C.long_causal_qkv(d)
    return causal_ref(qkv.double().numpy(), 3, C.LONG_LENGTHS), float(qkv[..., 2 * 3 * d:].abs().max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [32, 64])
def test_causal_attention_long_sequences(d, dtype):
    """B 8, H 3, T 300 (three query blocks, five key tiles), lengths 300, 257, 256, 129, 128, 97, 64 and 0"""
    from unispeech_amd import ops
    H, lengths = 3, list(C.LONG_LENGTHS)
    qkv = C.long_causal_qkv(d).to(dtype).cuda()
    il = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    o = ops.attn_causal_fwd(qkv, H, il)
    want, vmax = long_causal_ref(d)
    err = np.abs(f64(o) - want).max()
    print("causal attention T 300", dtype, d, "error", err, "of |V| max", vmax, "=", err / vmax, "bound", kernel_tol(dtype))
    assert np.isfinite(f64(o)).all() and err <= kernel_tol(dtype) * vmax, (err, vmax)
    for b, L in enumerate(lengths):                                              # rows at or beyond a length are zero
        assert not f64(o[b, L:]).any()
    poisoned = qkv.clone()                                                       # NaN and Inf behind every length change no bit
    for b, L in enumerate(lengths):
        poisoned[b, L:] = float("nan") if b % 2 else float("inf")
    assert torch.equal(bits(ops.attn_causal_fwd(poisoned, H, il)), bits(o))
    alone = ops.attn_causal_fwd(qkv[1:2, :257].contiguous(), H, il[1:2].contiguous())
    assert torch.equal(bits(alone[0]), bits(o[1, :257]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [32, 64])
def test_causal_attention_clamps_lengths(d, dtype):
    """a length above T counts as T and a negative one as 0"""
    from unispeech_amd import ops
    qkv, H, _ = causal_case(d, dtype)
    qkv = qkv[:2].contiguous()
    o = ops.attn_causal_fwd(qkv, H, torch.tensor([999, -5], dtype=torch.int32, device="cuda"))
    same = ops.attn_causal_fwd(qkv, H, torch.tensor([130, 0], dtype=torch.int32, device="cuda"))
    assert torch.equal(bits(o), bits(same)) and not f64(o[1]).any()
    vmax = np.abs(f64(qkv[..., 2 * H * d:])).max()
    assert np.abs(f64(o) - causal_ref(f64(qkv), H, [130, 0])).max() <= kernel_tol(dtype) * vmax


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [32, 64])
def test_causal_attention_rescales_under_rising_scores(d, dtype):
    """scores that rise by 0.5 from one 32-key step to the next in heads 0 and 2 (and fall in heads 1 and 3): the running maximum
    is renewed at nearly every step while the earlier steps keep most of the mass (tests/test_transformer_lm.py), so a kernel
    that does not rescale its sum or its output by exp(m_old - m_new) misses the bound"""
    from unispeech_amd import ops
    qkv = C.rising_causal_qkv(d).to(dtype).cuda()
    o = ops.attn_causal_fwd(qkv, C.RISING_H)
    want = causal_ref(f64(qkv), C.RISING_H, [C.RISING_T] * C.RISING_B)
    vmax = np.abs(f64(qkv[..., 2 * C.RISING_H * d:])).max()
    err = np.abs(f64(o) - want).max()
    print("rising scores", dtype, d, "error", err, "of |V| max", vmax, "=", err / vmax, "bound", kernel_tol(dtype))
    assert np.isfinite(f64(o)).all() and err <= kernel_tol(dtype) * vmax, (err, vmax)


@pytest.mark.parametrize("dtype", DTYPES)
def test_causal_attention_head_decomposition_at_scale(dtype):
    """B 4095, H 16, T 1, d 32 (B * H = 65 520, below the grid's 65 535): a single key, so every output row is its V row"""
    from unispeech_amd import ops
    B, H, d = 4095, 16, 32
    qkv = torch.randn(B, 1, 3 * H * d, generator=torch.Generator().manual_seed(65520)).to(dtype).cuda()
    o = ops.attn_causal_fwd(qkv, H)
    assert o.shape == (B, 1, H * d) and torch.equal(bits(o), bits(qkv[..., 2 * H * d:].contiguous()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_causal_attention_refuses_bad_arguments(dtype):
    """-1 before any launch: B * H = 65 536, qkv == O, a pointer off by 4 bytes, T, B or H of 0.  The buffers are as large as the
    largest geometry asked for."""
    from unispeech_amd import _lib, ops
    h = _lib.lib()
    d, p = 32, ops.ptr
    qkv = torch.zeros(4096 * 16 * 3 * d + 8, dtype=dtype, device="cuda")
    out = torch.full((4096 * 16 * d + 8,), 7.0, dtype=dtype, device="cuda")
    il = torch.ones(4096 + 1, dtype=torch.int32, device="cuda")
    off = 4 // qkv.element_size()

    def call(q=p(qkv), o=p(out), L=p(il), B=2, H=2, T=3):
        return h.wavlm_attn_causal_fwd(q, o, L, B, H, T, d, ops.dt(qkv), ctypes.c_float(d ** -0.5), ops.stream())
    assert call() == 0
    assert call(B=4095, H=16, T=1) == 0
    out.fill_(7.0)
    torch.cuda.synchronize()
    assert call(B=4096, H=16, T=1) == -1 and call(B=65536, H=1, T=1) == -1
    assert call(o=p(qkv)) == -1
    assert call(q=p(qkv, off)) == -1 and call(o=p(out, off)) == -1 and call(L=p(il.view(torch.int16), 1)) == -1
    assert call(T=0) == -1 and call(B=0) == -1 and call(H=0) == -1 and call(T=-1) == -1
    assert call(q=None) == -1 and call(o=None) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                    # nothing was launched


# ---------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def g():
    return load_golden("transformer_lm.npz")


def model_error(g, name, lp, tot):
    want = g[name + "/logprobs"]
    lp = lp.numpy()
    fin = np.isfinite(want)
    assert lp.shape == want.shape and np.array_equal(np.isfinite(lp), fin)
    assert tot[2] == -math.inf and lp[2, 3] == -math.inf
    assert np.allclose(tot.numpy()[[0, 1, 3]], lp[[0, 1, 3]].sum(1), rtol=1e-6)
    return np.abs(lp[fin] - want[fin]).max() / float(g[name + "/max"])


@pytest.mark.parametrize("name", list(C.MODELS))
def test_model_fp32_mode_against_the_fixture(g, name):
    m = C.build(name, torch.float32, "cuda")
    lp, tot = m.score(C.sentences())
    err = model_error(g, name, lp, tot)
    print("model %s fp32 mode: error %.3e of the max magnitude (bound %.1e)" % (name, err, HEAD_TOL))
    assert err <= HEAD_TOL
    # batch independence: other company, another order, one sentence per batch
    s = C.sentences()
    lp2, _ = m.score([s[3], s[1]])
    assert np.abs(lp2[0].numpy() - lp[3].numpy()).max() <= HEAD_TOL * float(g[name + "/max"])
    m.max_tokens = 1
    lp3, _ = m.score(s)
    fin = np.isfinite(lp.numpy())
    assert np.abs(lp3.numpy()[fin] - lp.numpy()[fin]).max() <= HEAD_TOL * float(g[name + "/max"])
    assert m.batches([len(x) + 1 for x in s]) == [[0], [1], [2], [3]]


@pytest.mark.parametrize("name", list(C.MODELS))
def test_model_bf16_mode_within_twice_the_reference_bf16_error(g, name, monkeypatch):
    m = C.build(name, torch.bfloat16, "cuda")
    lp, tot = m.score(C.sentences())
    err, e_ref = model_error(g, name, lp, tot), float(g[name + "/e_ref"])
    print("model %s bf16 mode: error %.3e (2 e_ref %.3e)" % (name, err, 2 * e_ref))
    assert err <= 2 * e_ref
    monkeypatch.setenv("WAVLM_LM_LOGPROB_COMPOSED", "1")                         # the composed output layer: same bound
    lpc, totc = m.score(C.sentences())
    assert model_error(g, name, lpc, totc) <= 2 * e_ref


def test_only_rows_with_a_target_reach_the_output_layer(monkeypatch):
    from unispeech_amd import transformer_lm as T
    m = C.build("A", torch.float32, "cuda")
    rows = []
    real = T.lm_logprob
    monkeypatch.setattr(T, "lm_logprob", lambda x, w, t, **k: rows.append((x.shape[0], int((t < 0).sum()))) or real(x, w, t, **k))
    m.score(C.sentences())
    assert rows == [(sum(len(s) + 1 for s in C.sentences()), 0)]                 # one batch of 4 x 34 padded rows, 46 of them real


# ------------------------------------------------------------------------------------------ the model at production width
@pytest.fixture(scope="module")
def gw():
    return load_golden("transformer_lm_wide.npz")


WIDE_BATCHES = {None: [[0, 1, 2, 3, 4, 5]], 256: [[0, 1], [2, 3], [4], [5]]}    # max_tokens: TransformerLM.batches


def wide_model_error(gw, name, m, max_tokens):
    """models W and X: D 512 / 256 (ops.gemm takes the 256-wide ping-pong kernels from 256 rows on), T 127, 128, 129 and 201
    across the attention's 128-query block, V 5003 = three slabs of the output layer"""
    s = C.wide_sentences()
    if max_tokens is not None:
        m.max_tokens = max_tokens
    assert m.batches([len(x) + 1 for x in s]) == WIDE_BATCHES[max_tokens]
    lp, tot = m.score(s)
    want = gw[name + "/logprobs"]
    lp = lp.numpy()
    fin = np.isfinite(want)
    assert lp.shape == want.shape == (6, 201) and np.array_equal(np.isfinite(lp), fin)
    i, t = C.WIDE_UNK_AT
    assert tot[i] == -math.inf and lp[i, t] == -math.inf
    rest = [k for k in range(6) if k != i]
    assert np.allclose(tot.numpy()[rest], lp[rest].sum(1), rtol=1e-6)
    for k, x in enumerate(s):
        assert not lp[k, len(x) + 1:].any()
    return np.abs(lp[fin] - want[fin]).max() / float(gw[name + "/max"])


@pytest.mark.parametrize("max_tokens", [None, 256])
@pytest.mark.parametrize("name", list(C.WIDE_MODELS))
def test_wide_model_fp32_mode_against_the_fixture(gw, name, max_tokens):
    err = wide_model_error(gw, name, C.build_wide(name, torch.float32, "cuda"), max_tokens)
    print("model %s fp32 mode, max_tokens %s: error %.3e of the max magnitude (bound %.1e)" % (name, max_tokens, err, HEAD_TOL))
    assert err <= HEAD_TOL


@pytest.mark.parametrize("max_tokens", [None, 256])
@pytest.mark.parametrize("name", list(C.WIDE_MODELS))
def test_wide_model_bf16_mode_within_twice_the_reference_bf16_error(gw, name, max_tokens, monkeypatch):
    m = C.build_wide(name, torch.bfloat16, "cuda")
    err, e_ref = wide_model_error(gw, name, m, max_tokens), float(gw[name + "/e_ref"])
    print("model %s bf16 mode, max_tokens %s: error %.3e (2 e_ref %.3e)" % (name, max_tokens, err, 2 * e_ref))
    assert err <= 2 * e_ref
    monkeypatch.setenv("WAVLM_LM_LOGPROB_COMPOSED", "1")                         # the composed output layer: same bound
    errc = wide_model_error(gw, name, m, max_tokens)
    print("model %s bf16 mode, composed output layer: error %.3e" % (name, errc))
    assert errc <= 2 * e_ref


# ---------------------------------------------------------------------------------------------------------- rescoring
@pytest.mark.parametrize("dtype", DTYPES)
def test_rescoring_on_the_device(g, dtype):
    from unispeech_amd import ctc_lexicon as X
    x, il, d, lexicon, opts, lm_dict = C.rescoring()
    hyps = X.lexicon_beam_decode(x.transpose(0, 1).contiguous().cuda().transpose(0, 1), il, d, lexicon, lexicon.lm,
                                 normalized=True, **opts)
    assert opts["nbest"] == 8 and [len(h) for h in hyps] == [8, 8]
    kw = dict(first_pass_lm=lexicon.lm, lm_weight=opts["lm_weight"], word_score=opts["word_score"], **C.RESCORE_OPTS)
    got = X.rescore_nbest(hyps, C.build("A", dtype, "cuda"), lm_dict, **kw)
    want = X.rescore_reference(hyps, C.build("A"), lm_dict, **kw)
    tol_token = (HEAD_TOL if dtype == torch.float32 else 2 * float(g["A/e_ref"])) * float(g["A/max"])
    for b, (gb, wb) in enumerate(zip(got, want)):
        ref = {(tuple(e["words"]), tuple(e["tokens"])): e for e in wb}
        for e in gb:
            r = ref[(tuple(e["words"]), tuple(e["tokens"]))]
            assert e["first_pass_score"] == r["first_pass_score"]
            if r["score"] == -math.inf:
                assert e["score"] == -math.inf and e["lm_score"] == -math.inf
            else:
                bound = C.RESCORE_OPTS["rescore_weight"] * (len(e["words"]) + 1) * tol_token
                assert abs(e["score"] - r["score"]) <= bound, (b, e, r, bound)
        assert gb[0]["words"] == wb[0]["words"] and gb[0]["tokens"] == wb[0]["tokens"]           # the same winner
        first = [(tuple(h[0]), tuple(h[1])) for h in hyps[b]]
        assert first.index((tuple(gb[0]["words"]), tuple(gb[0]["tokens"]))) == int(g["rescore/order_%d" % b][0])
        assert [e["score"] for e in gb] == sorted((e["score"] for e in gb), reverse=True)


# ------------------------------------------------------------------------------------------------------ command lines
def test_command_lines_on_a_tiny_checkpoint(g, tmp_path, capsys):
    """`transformer_lm score` on the device, and `ctc_lexicon decode / score` with --rescore-lm, on the tiny CTC checkpoint of
    tests/test_ctc_lexicon_gpu.py and model A written as a checkpoint: the printed scores are rescore_reference's over the same
    n-best list within the rescoring bound"""
    from test_ctc_lexicon_gpu import E2E, _e2e_logits, _e2e_setup
    from unispeech_amd import ctc, ctc_lexicon as X, transformer_lm as T
    d, lexicon, loaded, wavs, labels, arpa = _e2e_setup(tmp_path)
    words = [w for w in lexicon.words if w != "<unk>"][:C.VOCAB - 4]
    (tmp_path / "lm.dict.txt").write_text("".join("%s 1\n" % w for w in words + ["pad%d" % i for i in range(C.VOCAB - 4 - len(words))]))
    torch.save({"cfg": dict(C.MODELS["A"]), "model": C.build("A").state_dict()}, str(tmp_path / "lm.pt"))
    lm_dict = ctc.LetterDictionary.load(str(tmp_path / "lm.dict.txt"))
    assert len(lm_dict) == C.VOCAB
    tol_token = HEAD_TOL * float(g["A/max"])
    # transformer_lm score
    (tmp_path / "text.txt").write_text("%s %s\n\n%s nosuchword\n" % (words[0], words[5], words[2]))
    assert T.main(["score", str(tmp_path / "lm.pt"), str(tmp_path / "lm.dict.txt"), str(tmp_path / "text.txt")]) == 0
    out = capsys.readouterr().out.splitlines()
    want = T.score_reference(C.build("A"), [[lm_dict.index(words[0]), lm_dict.index(words[5])], []])[1].tolist()
    assert len(out) == 4 and out[2].split("\t")[0] == "-inf" and out[3].startswith("corpus: 3 sentences, 4 scored tokens")
    assert abs(float(out[0].split("\t")[0]) - want[0]) <= 3 * tol_token + 1e-4
    assert abs(float(out[1].split("\t")[0]) - want[1]) <= tol_token + 1e-4
    # ctc_lexicon decode with rescoring
    single, batch, il = _e2e_logits(loaded, wavs)
    flags = ["--lexicon", str(tmp_path / "lex.txt"), "--lm", arpa, "--beam", "3", "--beam-size-token", "3", "--beam-threshold",
             "inf", "--lm-weight", "1.5", "--word-score", "-0.5", "--unk-weight", "-4", "--sil-weight", "-0.25", "--nbest", "3",
             "--rescore-lm", str(tmp_path / "lm.pt"), "--rescore-dict", str(tmp_path / "lm.dict.txt"), "--rescore-weight", "0.5",
             "--rescore-word-score", "0.25"]
    assert X.main(["decode", str(tmp_path / "ck.pt"), str(tmp_path / "dict.ltr.txt")] + wavs + flags) == 0
    out = capsys.readouterr().out.splitlines()
    k = 0
    for x in single:
        hyps = X.lexicon_beam_decode(x, None, d, lexicon, lexicon.lm, nbest=3, **E2E)
        ref = X.rescore_reference(hyps, C.build("A"), lm_dict, lexicon.lm, 1.5, -0.5, 0.5, 0.25)[0]
        by_text = {}
        for e in ref:
            by_text.setdefault(" ".join(e["words"]), []).append(e["score"])
        for _ in ref:
            score, text = out[k].split("\t")
            bound = 0.5 * (len(text.split()) + 1) * tol_token + 1e-4          # + the four printed decimals
            assert any(s == float(score) == -math.inf or abs(float(score) - s) <= bound for s in by_text[text]), (out[k], by_text)
            k += 1
    assert k == len(out)
    with pytest.raises(SystemExit):
        X.main(["decode", str(tmp_path / "ck.pt"), str(tmp_path / "dict.ltr.txt")] + wavs + flags[:-6])   # --rescore-lm alone
    capsys.readouterr()
    # score: reports the WER of the rescored first hypothesis
    argv = ["score", str(tmp_path / "ck.pt"), str(tmp_path / "dict.ltr.txt"), str(tmp_path / "t.tsv"), str(tmp_path / "t.ltr")]
    assert X.main(argv + flags) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1].split()
    hyps = X.lexicon_beam_decode(batch, il, d, lexicon, lexicon.lm, nbest=3, **E2E)
    ref = X.rescore_reference(hyps, C.build("A"), lm_dict, lexicon.lm, 1.5, -0.5, 0.5, 0.25)
    w_err = sum(ctc.edit_distance(r[0]["words"], ctc.post_process(d.string(labels[i]), "letter").split()) for r, i in zip(ref, (1, 0)))
    assert line[0] == "UER" and line[8] == "w_errors" and line[10:] == ["w_total", "4"]
    # the count itself where the float64 winner is clear of the runner-up by more than twice the rescoring bound
    clear = all(len(r) < 2 or r[0]["score"] - r[1]["score"] > 2 * 0.5 * (len(r[0]["words"]) + len(r[1]["words"]) + 2) * tol_token
                for r in ref)
    print("rescored WER line:", " ".join(line), "| float64 winner clear:", clear)
    if clear:
        assert line[9] == str(w_err)
