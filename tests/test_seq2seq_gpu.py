"""csrc/s2s.hip (wavlm_attn_cross_fwd, wavlm_beam_step) and unispeech_amd.seq2seq on the device.  Reads tests/golden/ only.

Kernel bounds: those of tests/test_lm_incremental_gpu.py, the same arithmetic class (fp32 products and softmax state, bf16 only in
the operands and the stored result): 5e-5 of max |V| in fp32, 5e-5 + 2^-8 in bf16.  Search step: candidates and their order equal
the float64 step's, scores within 1e-5 (the case builder separates neighbouring float64 scores by more than 1e-4 except in the tie
cases, whose integer logits tie exactly in either precision).  Model bounds: HEAD_TOL = 5e-4 of the fixture's largest magnitude in
fp32 mode, 2 x e_ref (the reference itself in bf16 on the CPU) in bf16 mode."""
import ctypes
import math

import numpy as np
import pytest
import torch

import seq2seq_cases as C
from conftest import load_golden

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
HEAD_TOL = C.HEAD_TOL


def kernel_tol(dtype):
    return C.CROSS_TOL_F32 + (C.CROSS_TOL_BF16 if dtype == torch.bfloat16 else 0.0)


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.fixture(scope="module")
def golden():
    return load_golden("seq2seq.npz")


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_memory_behind():
    import gc
    from unispeech_amd import ops
    saved = dict(ops._WS)
    yield
    torch.cuda.synchronize()
    ops._WS.clear()
    ops._WS.update(saved)
    gc.collect()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ wavlm_attn_cross_fwd
def padded(t, extra, fill=math.nan):
    """a device copy of t whose last dimension sits in rows `extra` elements longer (the padding holds `fill`)"""
    store = torch.full(t.shape[:-1] + (t.shape[-1] + extra,), fill, dtype=t.dtype, device="cuda")
    view = store[..., :t.shape[-1]]
    view.copy_(t)
    return view


def run_cross(q, kv, lengths, off, live, H, dtype, pad=True, **kw):
    from unispeech_amd import ops
    qd, kvd = q.to(dtype), kv.to(dtype)
    qd = padded(qd, 8) if pad else qd.cuda()
    kvd = padded(kvd, 16) if pad else kvd.cuda()
    out = padded(torch.full(q.shape, 7.0, dtype=dtype), 8, 7.0) if pad else None
    o = ops.attn_cross_fwd(qd, kvd, H, off.cuda(), None if lengths is None else lengths.cuda(), None if live is None else live.cuda(),
                           out=out, **kw)
    if pad:
        assert bool((out.as_strided((q.shape[0], 8), (out.stride(0), 1), out.storage_offset() + q.shape[1]) == 7.0).all())
    return o


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("d", [32, 64])
def test_cross_kernel_against_fp64(d, H, dtype):
    """18 sentences: the 15 lengths on and around the 32- / 64- / 128-key boundaries of the kernels, each with at least one live
    row, and three more of which two have no rows; groups of 0, 1, 5, 32, 33 and 70 rows, padded strides, dead rows, NaN behind
    every length and in every dead row; bf16-valued operands, so one float64 result serves both dtypes"""
    q, kv, lengths, off, live = C.cross_case(d, H)
    rows = [int(live[int(off[b]):int(off[b + 1])].gt(0).sum()) for b in range(len(lengths))]
    assert {int(n) for n, r in zip(lengths, rows) if r} == set(C.CROSS_LENGTHS[:15]) and rows.count(0) == 2
    want = C.cross_reference(q, kv, lengths, off, live, H).numpy()
    vmax = float(kv[..., H * d:].abs().max())
    qp, kvp = C.poison(q, kv, lengths, live)
    o = run_cross(qp, kvp, lengths, off, live, H, dtype)
    assert o.shape == q.shape and o.dtype == dtype and np.isfinite(f64(o)).all()
    err = np.abs(f64(o) - want).max()
    print("attn_cross", dtype, "d", d, "H", H, "error", err, "of |V| max", vmax, "=", err / vmax, "bound", kernel_tol(dtype))
    assert err <= kernel_tol(dtype) * vmax
    assert not f64(o)[(live <= 0).numpy()].any()                                   # a dead row is zeros
    # a single key returns its v, bitwise (sentence 0 is one frame long)
    o1 = run_cross(q[:1], kv[:1], lengths[:1], torch.tensor([0, 1], dtype=torch.int32), None, H, dtype)
    assert int(lengths[0]) == 1 and torch.equal(bits(o1[0]), bits(kv[0, 0, H * d:].to(dtype).cuda()))
    # a grid sized for groups of one row: the workgroups walk several tiles each, with the same bits
    o2 = run_cross(qp, kvp, lengths, off, live, H, dtype, max_group=1)
    assert torch.equal(bits(o2), bits(o))
    # no lengths: every sentence is Ts long
    o3 = run_cross(q, kv, None, off, live, H, dtype, pad=False)
    full = torch.full_like(lengths, kv.shape[1])
    assert np.abs(f64(o3) - C.cross_reference(q, kv, full, off, live, H).numpy()).max() <= kernel_tol(dtype) * vmax


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_kernel_long_source(dtype):
    d, H = 64, 2
    q, kv, lengths, off, live = C.cross_case(d, H, seed=1, holes=False, **C.CROSS_LONG)
    want = C.cross_reference(q, kv, lengths, off, live, H).numpy()
    vmax = float(kv[..., H * d:].abs().max())
    qp, kvp = C.poison(q, kv, lengths, live)
    o = run_cross(qp, kvp, lengths, off, live, H, dtype)
    err = np.abs(f64(o) - want).max()
    print("attn_cross Ts 1500", dtype, "error", err, "=", err / vmax, "of |V| max, bound", kernel_tol(dtype))
    assert np.isfinite(f64(o)).all() and err <= kernel_tol(dtype) * vmax


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [32, 64])
def test_cross_kernel_bitwise_claims(d, dtype):
    H = 3
    q, kv, lengths, off, live = C.cross_case(d, H, holes=False)
    o = run_cross(q, kv, lengths, off, None, H, dtype)
    assert torch.equal(bits(run_cross(q, kv, lengths, off, None, H, dtype)), bits(o))                 # two runs
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    # a row alone in its group == the same row among 5 and among 33 (sentence 9: length 128)
    g = torch.Generator().manual_seed(77 + d)
    rows = C.bf16_valued(1.5 * torch.randn(33, H * d, generator=g))
    s = slice(9, 10)
    alone = run_cross(rows[4:5], kv[s], lengths[s], i32(0, 1), None, H, dtype)
    among5 = run_cross(rows[:5], kv[s], lengths[s], i32(0, 5), None, H, dtype)
    among33 = run_cross(rows, kv[s], lengths[s], i32(0, 33), None, H, dtype)
    assert torch.equal(bits(alone[0]), bits(among5[4])) and torch.equal(bits(alone[0]), bits(among33[4]))
    assert torch.equal(bits(among5), bits(among33[:5]))
    # a sentence alone == the same sentence inside a batch of 3, whatever its place
    b3 = torch.tensor([2, 9, 14])
    inside = run_cross(torch.cat([rows[:7], rows[:5], rows[:2]]), kv[b3], lengths[b3], i32(0, 7, 12, 14), None, H, dtype)
    assert torch.equal(bits(inside[7:12]), bits(among5))
    first = run_cross(rows[:5], kv[torch.tensor([9, 2, 14])], lengths[torch.tensor([9, 2, 14])], i32(0, 5, 5, 5), None, H, dtype)
    assert torch.equal(bits(first), bits(among5))


def raw_cross(q, kv, lengths, off, live, o, H, d, dtype, R=None, B=None, Ts=None, ld_q=None, s_kv=None, ld_kv=None, ld_o=None,
              max_group=None, qp=None, kvp=None, op=None, offp=None):
    from unispeech_amd import _lib, ops
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    return _lib.lib().wavlm_attn_cross_fwd(
        qp if qp is not None else p(q), q.stride(0) if ld_q is None else ld_q, kvp if kvp is not None else p(kv),
        kv.stride(0) if s_kv is None else s_kv, kv.stride(1) if ld_kv is None else ld_kv, p(lengths),
        offp if offp is not None else p(off), p(live), op if op is not None else p(o), o.stride(0) if ld_o is None else ld_o,
        q.shape[0] if R is None else R, kv.shape[0] if B is None else B, kv.shape[1] if Ts is None else Ts, H, d,
        _lib.BF16 if dtype == torch.bfloat16 else _lib.F32, d ** -0.5, q.shape[0] if max_group is None else max_group, ops.stream())


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_kernel_refuses_what_it_cannot_take(dtype):
    H, d, R, B, Ts = 2, 32, 6, 2, 40
    D = H * d
    es = 2 if dtype == torch.bfloat16 else 4
    q = torch.randn(R, D, device="cuda").to(dtype)
    kv = torch.randn(B, Ts, 2 * D, device="cuda").to(dtype)
    o = torch.full((R, D), 7.0, device="cuda", dtype=dtype)
    off = torch.tensor([0, 3, 6], dtype=torch.int32, device="cuda")
    lengths = torch.tensor([40, 17], dtype=torch.int32, device="cuda")
    a = (q, kv, lengths, off, None, o, H, d, dtype)
    vp = ctypes.c_void_p
    bad = [dict(qp=vp(0)), dict(kvp=vp(0)), dict(op=vp(0)), dict(offp=vp(0)),
           dict(qp=vp(q.data_ptr() + es)), dict(kvp=vp(kv.data_ptr() + 8)), dict(op=vp(o.data_ptr() + 8)),
           dict(ld_q=D + 1), dict(ld_kv=2 * D + 2), dict(ld_o=D + 2), dict(s_kv=Ts * 2 * D + 1),
           dict(ld_q=D - 8), dict(ld_o=D - 8), dict(ld_kv=2 * D - 8), dict(s_kv=(Ts - 1) * 2 * D),
           dict(op=vp(q.data_ptr())), dict(op=vp(kv.data_ptr() + 64 * es)), dict(qp=vp(kv.data_ptr() + 2 * D * es)),
           dict(R=0), dict(B=0), dict(Ts=0), dict(max_group=0)]
    for kw in bad:
        assert raw_cross(*a, **kw) == -1, kw
    for hd in (48, 16, 128):
        assert raw_cross(q, kv, lengths, off, None, o, H, hd, dtype) == -1
    from unispeech_amd import _lib, ops
    assert _lib.lib().wavlm_attn_cross_fwd(q.data_ptr(), D, kv.data_ptr(), Ts * 2 * D, 2 * D, None, off.data_ptr(), None, o.data_ptr(),
                                           D, R, B, Ts, H, d, 2, 0.1, R, ops.stream()) == -1         # WL_I16 is no dtype of it
    # a grid beyond one dimension: B * H * tiles > 2^31 - 1 (nothing is launched, so no array needs to be that long; at such
    # sizes the byte ranges may be found to overlap first -- either way the answer is -1 before any launch)
    assert raw_cross(*a, B=65535, max_group=2 ** 31 - 1, R=2 ** 31 - 1, s_kv=kv.stride(0)) == -1
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                                                   # nothing was launched
    assert raw_cross(*a) == 0
    torch.cuda.synchronize()
    assert bool((o != 7.0).any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_kernel_answers_bad_offsets_with_nan(dtype):
    """offsets that fall (5 -> 3) and that end beyond R (9 > 8): no address is formed from them; the rows only such groups name
    are NaN, the rows only the sound group names are right, rows 3 and 4 -- named by the sound group and spanned by the bad pairs
    -- hold one or the other (two workgroups write them: unspecified which, as the header says), and nothing beyond row R - 1
    is written"""
    H, d, R = 2, 32, 8
    q, kv, lengths, _, _ = C.cross_case(d, H, Ts=50, lengths=(50, 20, 33), groups=(5, 0, 3), holes=False)
    off = torch.tensor([0, 5, 3, 9], dtype=torch.int32)
    store = torch.full((R + 4, H * d), 7.0, dtype=dtype, device="cuda")
    from unispeech_amd import ops
    o = ops.attn_cross_fwd(q.to(dtype).cuda(), kv.to(dtype).cuda(), H, off.cuda(), lengths.cuda(), out=store[:R])
    want = C.cross_reference(q[:5], kv[:1], lengths[:1], torch.tensor([0, 5]), None, H).numpy()
    vmax = float(kv[..., H * d:].abs().max())
    assert np.abs(f64(o[:3]) - want[:3]).max() <= kernel_tol(dtype) * vmax
    assert np.isnan(f64(o[5:])).all()
    mid = f64(o[3:5])
    assert (np.isnan(mid) | (np.abs(mid - want[3:5]) <= kernel_tol(dtype) * vmax)).all()
    assert bool((store[R:] == 7.0).all())


# ------------------------------------------------------------------------------------------------------ wavlm_beam_step
def run_beam(case, dtype=torch.float32):
    """one launch on a fresh state -> (state, everything it holds, on the host)"""
    from unispeech_amd import ops
    B, beam, step = 3, case["beam"], case["step"]
    st = ops.BeamState(B, beam, 12, C.EOS, "cuda")
    st.cum.copy_(case["cum"])
    st.n_live.copy_(torch.tensor(case["n_live"], dtype=torch.int32))
    st.n_fin.copy_(torch.tensor(case["n_fin"], dtype=torch.int32))
    anc = torch.zeros(B * beam, st.ld_anc, dtype=torch.int32)
    anc[:, :step] = (1000 + 16 * torch.arange(B * beam).view(-1, 1) + torch.arange(step).view(1, -1)).to(torch.int32)
    st.anc[step % 2].copy_(anc)
    st.anc[(step + 1) % 2].fill_(-7)
    st.lengths.fill_(-7)
    ops.beam_step(case["logits"].to(dtype).cuda(), st, case["V"], max_len=case["max_len"], min_len=case["min_len"], pad=C.PAD,
                  unk=C.UNK, eos=C.EOS, unk_penalty=case["unk_penalty"], step=step)
    cs, ci, cn = st.candidates()
    host = dict(cum=st.cum, n_live=st.n_live, tokens=st.tokens, lengths=st.lengths, slots=st.slots, anc=st.anc[(step + 1) % 2],
                tree_parent=st.tree_parent, tree_token=st.tree_token, tree_score=st.tree_score, fin_f=st.fin_f, fin_i=st.fin_i,
                n_fin=st.n_fin, finished=st.finished, cand_s=cs, cand_i=ci, cand_n=cn)
    return st, {k: v.cpu().clone() for k, v in host.items()}, anc


def close(a, b, tol=1e-5):
    return (a == b) or abs(a - b) <= tol


def check_beam(case, got, anc_in):
    B, beam, V, step = 3, case["beam"], case["V"], case["step"]
    want = C.beam_expected(case)
    done = 0
    for b, e in enumerate(want):
        rows = slice(b * beam, (b + 1) * beam)
        if e is None:                                                               # finished earlier: nothing lives, nothing moves
            assert int(got["n_live"][b]) == 0 and int(got["cand_n"][b]) == 0 and int(got["n_fin"][b]) == case["n_fin"][b]
            assert got["lengths"][rows].tolist() == [0] * beam
            continue
        cands = e["candidates"]
        assert int(got["cand_n"][b]) == len(cands) == min(2 * beam, case["n_live"][b] * V - 1)
        assert got["cand_i"][b, :len(cands)].tolist() == [i for _, i in cands], (b, case["kind"])
        for j, (s, _) in enumerate(cands):
            assert close(float(got["cand_s"][b, j]), s), (b, j, float(got["cand_s"][b, j]), s)
        here, nxt = (step * B + b) * beam, ((step + 1) * B + b) * beam
        n0 = case["n_fin"][b]
        assert int(got["n_fin"][b]) == n0 + len(e["finished"])
        for j, (score, raw, ss, k, length) in enumerate(e["finished"]):
            f = got["fin_f"][b, n0 + j].tolist()
            assert close(f[0], score) and close(f[1], raw) and close(f[2], ss)
            assert got["fin_i"][b, n0 + j].tolist() == [here + k, length]
        done += int(e["done"])
        assert int(got["n_live"][b]) == len(e["rows"])
        for kk in range(beam):
            r = b * beam + kk
            if kk < len(e["rows"]):
                k, tok, s, ss = e["rows"][kk]
                assert (int(got["tokens"][r]), int(got["lengths"][r]), int(got["slots"][r])) == (tok, step + 2, nxt + kk)
                assert close(float(got["cum"][r]), s)
                assert got["anc"][r, :step + 1].tolist() == anc_in[b * beam + k, :step].tolist() + [here + k]
                assert (int(got["tree_parent"][nxt + kk]), int(got["tree_token"][nxt + kk])) == (here + k, tok)
                assert close(float(got["tree_score"][nxt + kk]), ss)
            else:
                assert int(got["lengths"][r]) == 0 and float(got["cum"][r]) == -math.inf
    assert int(got["finished"]) == done


@pytest.mark.parametrize("V,beam,kind", C.beam_cases())
def test_beam_step_against_the_float64_step(V, beam, kind):
    case = C.beam_case(V, beam, kind)
    _, got, anc = run_beam(case)
    check_beam(case, got, anc)
    _, again, _ = run_beam(case)
    for k, v in got.items():                                                        # bit for bit
        assert torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v, again[k].view(torch.int32)
                           if v.dtype == torch.float32 else again[k]), k
    if kind == "ties":                                                              # integer logits are exact in bf16 as well
        _, b16, _ = run_beam(case, torch.bfloat16)
        check_beam(case, b16, anc)


def test_beam_step_does_not_depend_on_the_batch():
    """sentence 2 of a batch of 3 == the same sentence alone (B = 1): candidates, scores and rows bit for bit"""
    from unispeech_amd import ops
    case = C.beam_case(2049, 5, "later")
    _, got, anc = run_beam(case)
    beam, step, V = 5, case["step"], case["V"]
    st = ops.BeamState(1, beam, 12, C.EOS, "cuda")
    st.cum.copy_(case["cum"][2 * beam:])
    st.n_live.fill_(beam)
    st.n_fin.fill_(case["n_fin"][2])
    st.anc[step % 2].copy_(anc[2 * beam:])
    ops.beam_step(case["logits"][2 * beam:].cuda(), st, V, max_len=case["max_len"], min_len=case["min_len"], pad=C.PAD, unk=C.UNK,
                  eos=C.EOS, unk_penalty=case["unk_penalty"], step=step)
    cs, ci, cn = (t.cpu() for t in st.candidates())
    assert int(cn[0]) == int(got["cand_n"][2]) and torch.equal(ci[0], got["cand_i"][2])
    assert torch.equal(cs[0].view(torch.int32), got["cand_s"][2].view(torch.int32))
    assert torch.equal(st.cum.cpu().view(torch.int32), got["cum"][2 * beam:].view(torch.int32))
    assert torch.equal(st.tokens.cpu(), got["tokens"][2 * beam:])


def test_beam_step_refuses_what_it_cannot_take():
    from unispeech_amd import _lib, ops
    st = ops.BeamState(2, 5, 12, C.EOS, "cuda")
    logits = torch.zeros(10, 32, device="cuda")
    kw = dict(max_len=12, min_len=1, pad=C.PAD, unk=C.UNK, eos=C.EOS)
    with pytest.raises(_lib.WavlmHipError):
        ops.beam_step(logits, st, 32, temperature=0.0, **kw)
    with pytest.raises(_lib.WavlmHipError):
        ops.beam_step(logits, st, 1, **kw)
    with pytest.raises(ValueError):
        ops.beam_step(logits, st, 33, **kw)
    with pytest.raises(ValueError):
        ops.beam_step(logits, st, 32, step=13, **kw)
    torch.cuda.synchronize()
    assert int(st.finished.cpu()) == 0 and st.n_live.cpu().tolist() == [1, 1] and st.step == 0


# ------------------------------------------------------------------------------------------------------------- the model
def hyps_of(golden, name, beam):
    p = "%s/beam%d/" % (name, beam)
    return golden[p + "tokens"], golden[p + "lens"], golden[p + "score"], golden[p + "pos"]


@pytest.mark.parametrize("name", list(C.MODELS))
def test_model_fp32_mode(golden, name):
    """teacher-forced logits against the golden; every step's logits of the search against the teacher-forced ones of the
    hypothesis it returned; generate() returns the golden hypotheses at both beams"""
    from unispeech_amd import seq2seq as S
    m = C.build(name, torch.float32, "cuda")
    src, pm = C.batch()
    src, pm = src.cuda(), pm.cuda()
    mx = float(golden[name + "/max"])
    logits = m(src, pm, C.forced_tokens())
    err = np.abs(f64(logits) - golden[name + "/logits"]).max()
    print("seq2seq", name, "fp32 teacher-forced error", err, "=", err / mx, "of max, bound", HEAD_TOL)
    assert logits.shape == (3, 9, C.VOCAB) and logits.dtype == torch.float32 and err <= HEAD_TOL * mx
    for beam in C.BEAMS:
        steps, reads = [], []
        orig = S.read_device
        S.read_device = lambda t: (reads.append(1), orig(t))[1]
        try:
            res = m.generate(src, pm, beam=beam, max_len_b=C.MAX_LEN_B, step_logits=steps)
        finally:
            S.read_device = orig
        assert len(reads) == m.loop_reads <= math.ceil(len(steps) / 8) + 1 and len(steps) <= C.MAX_LEN_B + 1
        toks, lens, score, pos = hyps_of(golden, name, beam)
        worst = 0.0
        for b in range(3):
            assert len(res[b]) == int((lens[b] > 0).sum())
            for j, h in enumerate(res[b]):
                n = int(lens[b, j])
                assert h["tokens"].tolist() == toks[b, j, :n].tolist(), (name, beam, b, j)
                tol = HEAD_TOL * (n + 1) * mx
                assert abs(float(h["score"]) - float(score[b, j])) <= tol
                assert np.abs(h["positional_scores"].numpy() - pos[b, j, :n]).max() <= tol
                worst = max(worst, abs(float(h["score"]) - float(score[b, j])))
        print("seq2seq", name, "beam", beam, "steps", len(steps), "host reads", len(reads), "largest score difference", worst)
        if beam == 1:
            # row b of step t held the prefix of sentence b's only hypothesis: its logits are the teacher-forced ones
            prev = torch.full((3, C.MAX_LEN_B + 1), C.PAD, dtype=torch.long)
            for b in range(3):
                n = int(lens[b, 0])
                prev[b, 0] = C.EOS
                prev[b, 1:n] = torch.from_numpy(toks[b, 0, :n - 1])
            forced = f64(m(src, pm, prev))
            fmax, worst = np.abs(forced).max(), 0.0
            for t, (lg, ln) in enumerate(steps):
                for b in range(3):
                    if int(ln[b]) > 0:
                        assert t < int(lens[b, 0])
                        worst = max(worst, np.abs(f64(lg[b]) - forced[b, t]).max())
            print("seq2seq", name, "step-by-step against teacher-forced", worst, "=", worst / fmax, "bound", kernel_tol(torch.float32))
            assert worst <= kernel_tol(torch.float32) * fmax


@pytest.mark.parametrize("name", list(C.MODELS))
def test_model_bf16_mode(golden, name):
    """logits within 2 e_ref of the golden; the float64 objective of each returned 1-best equals its returned score within the
    tolerance and lies within twice the tolerance of the float64 optimum.  The winner's identity is not asserted."""
    from unispeech_amd import seq2seq as S
    m = C.build(name, torch.bfloat16, "cuda")
    ref = C.build(name)
    src, pm = C.batch()
    mx, e_ref = float(golden[name + "/max"]), float(golden[name + "/e_ref"])
    logits = m(src.cuda().to(torch.bfloat16), pm.cuda(), C.forced_tokens())
    err = np.abs(f64(logits) - golden[name + "/logits"]).max()
    print("seq2seq", name, "bf16 teacher-forced error", err, "=", err / mx, "of max, bound", 2 * e_ref)
    assert err <= 2 * e_ref * mx
    enc = S.encoder_proj_reference(ref, torch.from_numpy(golden["enc/x"]))
    fpm = torch.from_numpy(golden["enc/padding_mask"])
    res = m.generate(src.cuda().to(torch.bfloat16), pm.cuda(), beam=5, max_len_b=C.MAX_LEN_B)
    _, _, score, _ = hyps_of(golden, name, 5)
    for b in range(3):
        assert res[b] and [float(h["score"]) for h in res[b]] == sorted((float(h["score"]) for h in res[b]), reverse=True)
        h = res[b][0]
        toks = h["tokens"].tolist()
        n = len(toks)
        assert toks[-1] == C.EOS and C.PAD not in toks and 1 <= n <= C.MAX_LEN_B + 1
        prev = torch.tensor([[C.EOS] + toks[:-1]])
        lp = torch.log_softmax(S.decoder_reference(ref, enc[b:b + 1], fpm[b:b + 1], prev)[0], -1)
        obj = float(lp[torch.arange(n), torch.tensor(toks)].sum()) / n
        tol = 2 * e_ref * (n + 1) * mx
        print("seq2seq", name, "bf16 sentence", b, "returned %.4f, float64 objective %.4f, float64 optimum %.4f (tol %.4f)"
              % (float(h["score"]), obj, float(score[b, 0]), tol))
        assert abs(obj - float(h["score"])) <= tol and float(score[b, 0]) - obj <= 2 * tol
