"""wavlm_beam_step_fused (csrc/s2s.hip) and the fused search (unispeech_amd.sequence_generator) on the device.  Reads tests/golden/
only.

Step bound: candidates, rows, tree, ancestors and finished lists equal the float64 step's exactly; scores within 1e-5 (1 +
|lm_weight|) -- the bound of tests/test_seq2seq_gpu.py per log-softmax term, of which the fused score holds 1 + |lm_weight| (the
builder separates neighbouring float64 scores by more than 1e-4 (1 + |lm_weight|)).  The worst error seen is printed.  Model
bounds: HEAD_TOL (n + 1) (mx + |lm_weight| lm_mx) in fp32 mode, 2 (n + 1) (e_ref mx + |lm_weight| lm_e_ref lm_mx) in bf16 mode;
the LM's step logits against the golden's teacher-forced ones within the fp32 kernel bound of tests/test_lm_incremental_gpu.py
(5e-5 of the largest magnitude)."""
import math

import numpy as np
import pytest
import torch

import seq2seq_cases as C
import seq2seq_fusion_cases as F
from conftest import load_golden

pytestmark = pytest.mark.gpu

HEAD_TOL = C.HEAD_TOL
F32_TOL = 5e-5                          # tests/test_lm_incremental_gpu.py
WORST = {"err": 0.0}                    # the largest score error seen, as a share of its bound


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def golden():
    return load_golden(F.GOLDEN)


@pytest.fixture(scope="module")
def plain():
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


# ------------------------------------------------------------------------------------------------ wavlm_beam_step_fused
def make_state(case, sentences=(0, 1, 2)):
    """a BeamState holding the case's sentences `sentences`: the slot of position j of row r is j * R + r, tree_token holds the
    histories, anc the slots of positions 0 .. step - 1 -> (state, the ancestors on the host)"""
    from unispeech_amd import ops
    beam, step = case["beam"], case["step"]
    B = len(sentences)
    R = B * beam
    rows = torch.cat([torch.arange(b * beam, (b + 1) * beam) for b in sentences])
    st = ops.BeamState(B, beam, case["max_len"], C.EOS, "cuda")
    st.cum.copy_(case["cum"][rows])
    st.n_live.copy_(torch.tensor([case["n_live"][b] for b in sentences], dtype=torch.int32))
    st.n_fin.copy_(torch.tensor([case["n_fin"][b] for b in sentences], dtype=torch.int32))
    hist = case["hist"][rows]
    anc = torch.zeros(R, st.ld_anc, dtype=torch.int32)
    anc[:, :step] = (torch.arange(step).view(1, -1) * R + torch.arange(R).view(-1, 1)).to(torch.int32)
    tree = st.tree_token.cpu()
    tree[:(step + 1) * R] = hist.t().reshape(-1).to(torch.int32)
    st.tree_token.copy_(tree)
    st.tokens.copy_(hist[:, step].to(torch.int32))
    st.slots.copy_((step * R + torch.arange(R)).to(torch.int32))
    st.anc[step % 2].copy_(anc)
    st.anc[(step + 1) % 2].fill_(-7)
    st.lengths.fill_(-7)
    return st, anc, rows


def snapshot(st, step):
    cs, ci, cn = st.candidates()
    host = dict(cum=st.cum, n_live=st.n_live, tokens=st.tokens, lengths=st.lengths, slots=st.slots, anc=st.anc[(step + 1) % 2],
                tree_parent=st.tree_parent, tree_token=st.tree_token, tree_score=st.tree_score, fin_f=st.fin_f, fin_i=st.fin_i,
                n_fin=st.n_fin, finished=st.finished, cand_s=cs, cand_i=ci, cand_n=cn)
    return {k: v.cpu().clone() for k, v in host.items()}


def run_fused(case, dtype=torch.float32, lm_dtype=torch.float32, sentences=(0, 1, 2)):
    """one launch on a fresh state -> (everything the state holds, the ancestors it read, the consumed logits), on the host"""
    from unispeech_amd import ops
    st, anc, rows = make_state(case, sentences)
    logits = case["logits"][rows].to(dtype).cuda()
    lm = None if case["lm"] is None else case["lm"][rows].to(lm_dtype).cuda()
    ops.beam_step_fused(logits, st, case["V"], max_len=case["max_len"], min_len=case["min_len"], pad=C.PAD, unk=C.UNK, eos=C.EOS,
                        lm_logits=lm, lm_weight=case["lm_weight"], no_repeat_ngram_size=case["n"],
                        unk_penalty=case["unk_penalty"], step=case["step"])
    return snapshot(st, case["step"]), anc, logits.float().cpu()


def close(a, b, tol):
    if a == b:
        return True
    WORST["err"] = max(WORST["err"], abs(a - b) / tol) if math.isfinite(a - b) else math.inf
    return abs(a - b) <= tol


def check_fused(case, got, anc_in):
    B, beam, V, step = 3, case["beam"], case["V"], case["step"]
    tol = 1e-5 * (1 + abs(case["lm_weight"]))
    want = F.fused_expected(case)
    done = 0
    for b, e in enumerate(want):
        rows = slice(b * beam, (b + 1) * beam)
        if e is None:                                                               # finished earlier: nothing lives, nothing moves
            assert int(got["n_live"][b]) == 0 and int(got["cand_n"][b]) == 0 and int(got["n_fin"][b]) == case["n_fin"][b]
            assert got["lengths"][rows].tolist() == [0] * beam
            continue
        cands = e["candidates"]
        assert int(got["cand_n"][b]) == len(cands) == min(2 * beam, case["n_live"][b] * V - 1)
        assert got["cand_i"][b, :len(cands)].tolist() == [i for _, i in cands], b
        for j, (s, _) in enumerate(cands):
            assert close(float(got["cand_s"][b, j]), s, tol), (b, j, float(got["cand_s"][b, j]), s)
        here, nxt = (step * B + b) * beam, ((step + 1) * B + b) * beam
        n0 = case["n_fin"][b]
        assert int(got["n_fin"][b]) == n0 + len(e["finished"])
        for j, (score, raw, ss, k, length) in enumerate(e["finished"]):
            f = got["fin_f"][b, n0 + j].tolist()
            assert close(f[0], score, tol) and close(f[1], raw, tol) and close(f[2], ss, tol)
            assert got["fin_i"][b, n0 + j].tolist() == [here + k, length]
        done += int(e["done"])
        assert int(got["n_live"][b]) == len(e["rows"])
        for kk in range(beam):
            r = b * beam + kk
            if kk < len(e["rows"]):
                k, tok, s, ss = e["rows"][kk]
                assert (int(got["tokens"][r]), int(got["lengths"][r]), int(got["slots"][r])) == (tok, step + 2, nxt + kk)
                assert close(float(got["cum"][r]), s, tol)
                assert got["anc"][r, :step + 1].tolist() == anc_in[b * beam + k, :step].tolist() + [here + k]
                assert (int(got["tree_parent"][nxt + kk]), int(got["tree_token"][nxt + kk])) == (here + k, tok)
                assert close(float(got["tree_score"][nxt + kk]), ss, tol)
            else:
                assert int(got["lengths"][r]) == 0 and float(got["cum"][r]) == -math.inf
    assert int(got["finished"]) == done


def same_bits(a, b):
    for k, v in a.items():
        x, y = (v.view(torch.int32), b[k].view(torch.int32)) if v.dtype == torch.float32 else (v, b[k])
        assert torch.equal(x, y), k


def written(before, after):
    """the entries of the logits the call changed (NaN-aware, by bits)"""
    return (before.view(torch.int32) != after.view(torch.int32)).numpy()


@pytest.mark.parametrize("V,beam,n,w,step", F.fused_cases())
def test_fused_step_against_the_float64_step(V, beam, n, w, step):
    case = F.fused_case(V, beam, n, w, step)
    assert case["sensitive"] == F.ban_possible(n, step)
    got, anc, consumed = run_fused(case)
    check_fused(case, got, anc)
    # the logits are consumed: exactly the banned entries of the live rows became -inf, nothing else was written
    banned = F.fused_banned(case)
    before = case["logits"].clone()
    changed = written(before, consumed)
    assert bool((consumed.numpy()[banned] == -math.inf).all())
    assert np.array_equal(changed, banned & (before.numpy() != -math.inf))
    again, _, _ = run_fused(case)
    same_bits(got, again)                                                           # bit for bit
    print("fused step V=%d beam=%d n=%d w=%r step=%d: worst score error so far %.3f of the bound" % (V, beam, n, w, step, WORST["err"]))
    assert WORST["err"] <= 1.0


@pytest.mark.parametrize("dtype,lm_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                            (torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)])
@pytest.mark.parametrize("V,beam,n", [(32, 5, 2), (2049, 32, 3), (2049, 1, 0)])
def test_fused_step_ties(V, beam, n, dtype, lm_dtype):
    """integer logits (exact in bf16 as well) and an integer weight: scores tie exactly, the order is the tie rule's"""
    case = F.fused_case(V, beam, n, 2.0, 11, ties=True)
    got, anc, consumed = run_fused(case, dtype, lm_dtype)
    check_fused(case, got, anc)
    assert np.array_equal(written(case["logits"].clone(), consumed), F.fused_banned(case))


def test_fused_step_does_not_depend_on_the_batch():
    """sentence 2 of a batch of 3 == the same sentence alone (B = 1), bit for bit"""
    case = F.fused_case(2049, 5, 3, 0.7, 11)
    got, _, consumed = run_fused(case)
    alone, _, consumed1 = run_fused(case, sentences=(2,))
    beam = 5
    assert int(alone["cand_n"][0]) == int(got["cand_n"][2]) and torch.equal(alone["cand_i"][0], got["cand_i"][2])
    assert torch.equal(alone["cand_s"][0].view(torch.int32), got["cand_s"][2].view(torch.int32))
    assert torch.equal(alone["cum"].view(torch.int32), got["cum"][2 * beam:].view(torch.int32))
    assert torch.equal(alone["tokens"], got["tokens"][2 * beam:])
    assert torch.equal(alone["fin_f"][0].view(torch.int32), got["fin_f"][2].view(torch.int32))
    assert torch.equal(consumed1.view(torch.int32), consumed[2 * beam:].view(torch.int32))


@pytest.mark.parametrize("V,beam,kind", C.beam_cases())
def test_without_lm_and_blocker_the_step_is_beam_step(V, beam, kind):
    """lm_logits None, n = 0: every output array equals ops.beam_step's bit for bit, and the logits stay as they were"""
    from unispeech_amd import ops
    case = C.beam_case(V, beam, kind)
    B, step = 3, case["step"]
    out = []
    for fused in (False, True):
        for dtype in ((torch.float32, torch.bfloat16) if kind == "ties" else (torch.float32,)):
            st = ops.BeamState(B, beam, 12, C.EOS, "cuda")
            st.cum.copy_(case["cum"])
            st.n_live.copy_(torch.tensor(case["n_live"], dtype=torch.int32))
            st.n_fin.copy_(torch.tensor(case["n_fin"], dtype=torch.int32))
            anc = torch.zeros(B * beam, st.ld_anc, dtype=torch.int32)
            anc[:, :step] = (16 * torch.arange(B * beam).view(-1, 1) % 7 + torch.arange(step).view(1, -1)).to(torch.int32)
            st.anc[step % 2].copy_(anc)
            st.anc[(step + 1) % 2].fill_(-7)
            st.lengths.fill_(-7)
            logits = case["logits"].to(dtype).cuda()
            kw = dict(max_len=case["max_len"], min_len=case["min_len"], pad=C.PAD, unk=C.UNK, eos=C.EOS,
                      unk_penalty=case["unk_penalty"], step=step)
            if fused:
                ops.beam_step_fused(logits, st, V, **kw)
                assert torch.equal(logits.cpu().view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                   case["logits"].to(dtype).view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
            else:
                ops.beam_step(logits, st, V, **kw)
            out.append(snapshot(st, step))
    half = len(out) // 2
    for a, b in zip(out[:half], out[half:]):
        same_bits(a, b)


def test_fused_step_refuses_what_it_cannot_take():
    from unispeech_amd import _lib, ops
    st = ops.BeamState(2, 5, 12, C.EOS, "cuda")
    logits = torch.zeros(10, 32, device="cuda")
    lm = torch.zeros(10, 36, device="cuda")
    kw = dict(max_len=12, min_len=1, pad=C.PAD, unk=C.UNK, eos=C.EOS)
    before = snapshot(st, 0)
    for bad in (dict(temperature=0.0), dict(no_repeat_ngram_size=-1), dict(lm_logits=lm, lm_weight=math.inf),
                dict(lm_weight=math.nan), dict(lm_weight=-math.inf),
                dict(lm_logits=logits)):                                            # the LM's logits overlap the consumed buffer
        with pytest.raises(_lib.WavlmHipError):
            ops.beam_step_fused(logits, st, 32, **dict(kw, **bad))
    with pytest.raises(_lib.WavlmHipError):
        ops.beam_step_fused(logits, st, 1, **kw)
    with pytest.raises(ValueError):
        ops.beam_step_fused(logits, st, 32, lm_logits=lm[:, :31], **kw)            # narrower than V
    with pytest.raises(ValueError):
        ops.beam_step_fused(logits, st, 33, **kw)
    with pytest.raises(ValueError):
        ops.beam_step_fused(logits, st, 32, step=13, **kw)
    # through the C interface: ld_lm < V and a misaligned lm_logits
    L = _lib.lib()

    def call(lm_ptr, ld_lm, lm_dt):
        p = ops.ptr
        return L.wavlm_beam_step_fused(p(logits), 32, ops.F32, lm_ptr, ld_lm, lm_dt, 1.0, 0, p(st.cum), p(st.n_live), p(st.tokens),
                                       p(st.lengths), p(st.slots), p(st.anc[0]), p(st.anc[1]), st.ld_anc, p(st.tree_parent),
                                       p(st.tree_token), p(st.tree_score), st.tree_slots, p(st.fin_f), p(st.fin_i), p(st.n_fin),
                                       p(st.finished), st.B, st.beam, 32, 0, 12, 1, C.PAD, C.UNK, C.EOS, 0.0, 1.0, 1.0, 1, p(st.ws),
                                       st.ws.numel(), ops.stream())
    assert call(ops.ptr(lm), 31, ops.F32) != 0
    assert call(ops.ptr(lm.view(torch.uint8), 2), 36, ops.F32) != 0
    assert call(ops.ptr(lm.view(torch.uint8), 1), 72, ops.BF16) != 0
    assert call(ops.ptr(lm), 36, 7) != 0
    torch.cuda.synchronize()
    same_bits(before, snapshot(st, 0))
    assert st.step == 0 and bool((logits == 0).all())


# ------------------------------------------------------------------------------------------------------------- the model
class _Dict:
    def __len__(self):
        return C.VOCAB

    def pad(self):
        return C.PAD

    def eos(self):
        return C.EOS

    def unk(self):
        return C.UNK


def generator(model, lm, o, beam):
    from unispeech_amd.sequence_generator import SequenceGenerator
    return SequenceGenerator([model], _Dict(), beam_size=beam, max_len_b=C.MAX_LEN_B, lm_model=lm if o["lm"] else None,
                             lm_weight=o["lm_weight"], no_repeat_ngram_size=o["no_repeat_ngram_size"])


@pytest.mark.parametrize("name", list(C.MODELS))
def test_model_fp32_mode(golden, plain, name):
    """SequenceGenerator returns the golden hypotheses of every option set at both beams; the host reads stay those of the unfused
    search; at beam 1 every step's LM logits are the golden's teacher-forced ones"""
    from unispeech_amd import seq2seq as S
    m, lm = C.build(name, torch.float32, "cuda"), F.build_lm(name, torch.float32, "cuda")
    src, pm = C.batch()
    sample = {"net_input": {"source": src.cuda(), "padding_mask": pm.cuda()}}
    mx, lm_mx = float(plain[name + "/max"]), float(golden[name + "/lm/max"])
    for sname, o in F.SETS.items():
        if name not in o["models"]:
            continue
        for beam in C.BEAMS:
            gen = generator(m, lm, o, beam)
            gen.step_logits = steps = []
            reads, orig = [], S.read_device
            S.read_device = lambda t: (reads.append(1), orig(t))[1]
            try:
                res = gen.generate([m], sample)
            finally:
                S.read_device = orig
            assert len(reads) == m.loop_reads <= math.ceil(len(steps) / 8) + 1 and len(steps) <= C.MAX_LEN_B + 1
            p = "%s/%s/beam%d/" % (name, sname, beam)
            toks, lens, score, pos = golden[p + "tokens"], golden[p + "lens"], golden[p + "score"], golden[p + "pos"]
            worst = 0.0
            for b in range(3):
                assert len(res[b]) == int((lens[b] > 0).sum())
                for j, h in enumerate(res[b]):
                    n = int(lens[b, j])
                    assert h["tokens"].tolist() == toks[b, j, :n].tolist(), (name, sname, beam, b, j)
                    tol = HEAD_TOL * (n + 1) * (mx + abs(o["lm_weight"]) * lm_mx * o["lm"])
                    assert abs(float(h["score"]) - float(score[b, j])) <= tol
                    assert np.abs(h["positional_scores"].numpy() - pos[b, j, :n]).max() <= tol
                    worst = max(worst, abs(float(h["score"]) - float(score[b, j])))
            print("fused seq2seq", name, sname, "beam", beam, "steps", len(steps), "host reads", len(reads),
                  "largest score difference", worst)
            if beam == 1 and o["lm"]:
                want, worst = golden[p + "lm_logits"].astype(np.float64), 0.0
                for t, (lg, ln, ll) in enumerate(steps):
                    assert ll is not None and ll.shape == (3, C.VOCAB) and ll.dtype == torch.float32
                    for b in range(3):
                        if int(ln[b]) > 0:
                            assert t < int(lens[b, 0])
                            worst = max(worst, np.abs(f64(ll[b]) - want[b, t]).max())
                print("fused seq2seq", name, sname, "LM step logits against teacher-forced", worst, "=", worst / lm_mx, "bound", F32_TOL)
                assert worst <= F32_TOL * lm_mx
            elif not o["lm"]:
                assert all(len(s) == 3 and s[2] is None for s in steps)


@pytest.mark.parametrize("name,sname", [(m, s) for s, o in F.SETS.items() if o["lm"] for m in o["models"]])
def test_model_bf16_mode(golden, plain, name, sname):
    """the float64 objective of each returned 1-best -- the model term plus lm_weight x the LM term, length-normalised -- equals
    the returned score within tol = 2 (n + 1) (e_ref mx + |lm_weight| lm_e_ref lm_mx) and lies within 2 tol of the float64 optimum
    of the same constrained search; under FN it holds no repeated 3-gram.  The winner's identity is not asserted."""
    from unispeech_amd import seq2seq as S
    from unispeech_amd.transformer_lm import _forward64
    o = F.SETS[sname]
    m, lm = C.build(name, torch.bfloat16, "cuda"), F.build_lm(name, torch.bfloat16, "cuda")
    ref, ref_lm = C.build(name), F.build_lm(name)
    src, pm = C.batch()
    mx, e_ref = float(plain[name + "/max"]), float(plain[name + "/e_ref"])
    lm_mx, lm_e = float(golden[name + "/lm/max"]), float(golden[name + "/lm/e_ref"])
    enc = S.encoder_proj_reference(ref, torch.from_numpy(plain["enc/x"]))
    fpm = torch.from_numpy(plain["enc/padding_mask"])
    res = generator(m, lm, o, 5).generate([m], {"net_input": {"source": src.cuda().to(torch.bfloat16), "padding_mask": pm.cuda()}})
    score = golden["%s/%s/beam5/score" % (name, sname)]
    w = o["lm_weight"]
    for b in range(3):
        assert res[b] and [float(h["score"]) for h in res[b]] == sorted((float(h["score"]) for h in res[b]), reverse=True)
        h = res[b][0]
        toks = h["tokens"].tolist()
        n = len(toks)
        assert toks[-1] == C.EOS and C.PAD not in toks and 1 <= n <= C.MAX_LEN_B + 1
        if o["no_repeat_ngram_size"]:
            assert not F.repeats(toks, o["no_repeat_ngram_size"])
        prev = torch.tensor([[C.EOS] + toks[:-1]])
        idx = (torch.arange(n), torch.tensor(toks))
        lp = torch.log_softmax(S.decoder_reference(ref, enc[b:b + 1], fpm[b:b + 1], prev)[0], -1)[idx]
        with torch.no_grad():
            ll = _forward64(ref_lm, toks[:-1])[idx]
        obj = float((lp + w * ll).sum()) / n
        tol = 2 * (n + 1) * (e_ref * mx + abs(w) * lm_e * lm_mx)
        print("fused seq2seq", name, sname, "bf16 sentence", b, "returned %.4f, float64 objective %.4f, float64 optimum %.4f "
              "(tol %.4f)" % (float(h["score"]), obj, float(score[b, 0]), tol))
        assert abs(obj - float(h["score"])) <= tol and float(score[b, 0]) - obj <= 2 * tol
