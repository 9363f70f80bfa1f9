"""csrc/lm_step.hip (wavlm_attn_step), TransformerLM.incremental() and ctc_lexicon.fused_lexicon_decode on the device.  Reads
tests/golden/ only.

Kernel bounds: the constants of the causal-attention tests of tests/test_transformer_lm_gpu.py, the same arithmetic class (fp32
products and softmax state, bf16 only in the operands and the stored result): 5e-5 of max |V| in fp32, 5e-5 + 2^-8 = 3.96e-3 in
bf16.  Model bounds: HEAD_TOL = 5e-4 of the fixture's largest magnitude in fp32 mode, 2 x e_ref (the reference itself in bf16 on
the CPU) in bf16 mode.  Search: see test_fused_search_*."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import lm_incremental_cases as I
import transformer_lm_cases as C
from conftest import load_golden

pytestmark = pytest.mark.gpu

F32_TOL, BF16_TOL, HEAD_TOL = 5e-5, 2.0 ** -8, I.HEAD_TOL          # tests/test_transformer_lm_gpu.py
DTYPES = [torch.float32, torch.bfloat16]


def kernel_tol(dtype):
    return F32_TOL + (BF16_TOL if dtype == torch.bfloat16 else 0.0)


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_memory_behind():
    import gc
    from unispeech_amd import ops
    saved = dict(ops._WS)
    yield
    torch.cuda.synchronize()
    ops._WS.clear()
    ops._WS.update(saved)
    for cached in (I.step_case, I.search_reference, I.search_emissions, C.rescoring, causal_ref_rows):
        cached.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- wavlm_attn_step
def run_step(case, dtype, kc=None, vc=None, rows=None, anc=None):
    """one launch on copies of the case's caches -> (O, kc, vc) on the device"""
    from unispeech_amd import ops
    dev = "cuda"
    kc = (case["kc"] if kc is None else kc).to(dtype).to(dev)
    vc = (case["vc"] if vc is None else vc).to(dtype).to(dev)
    sel = slice(None) if rows is None else rows
    anc = case["anc"] if anc is None else anc
    o = ops.attn_step(case["qkv"][sel].to(dtype).to(dev).contiguous(), kc, vc, case["slot"][sel].contiguous().to(dev),
                      anc[sel].contiguous().to(dev), case["lengths"][sel].contiguous().to(dev), case["H"], case["max_length"])
    return o, kc, vc


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R", [1, 7, 64, 65, 257])
@pytest.mark.parametrize("H", [1, 3, 16])
@pytest.mark.parametrize("d", [32, 64])
def test_step_kernel_against_fp64(d, H, R, dtype):
    """a random tree in a shuffled slot numbering, lengths 1 .. 300 with the neighbours of the 64-key pass boundaries, 0 and
    negative ones; bf16-valued operands, so one float64 result serves both dtypes"""
    case = I.step_case(d, H, R)
    o, kc, vc = run_step(case, dtype)
    D, L = H * d, case["lengths"].numpy()
    assert o.shape == (R, D) and o.dtype == dtype and np.isfinite(f64(o)).all()
    err = np.abs(f64(o) - case["out"]).max()
    print("attn_step", dtype, "d", d, "H", H, "R", R, "error", err, "of |V| max", case["vmax"], "=", err / case["vmax"],
          "bound", kernel_tol(dtype))
    assert err <= kernel_tol(dtype) * case["vmax"]
    qkv = case["qkv"].to(dtype).cuda()
    for r in range(R):
        if L[r] <= 0:
            assert not f64(o[r]).any()                                           # a skipped row is zeros
        if L[r] == 1:
            assert torch.equal(bits(o[r]), bits(qkv[r, 2 * D:]))                 # a single key: the row's own v, bitwise
    # the named slots hold the rows' k and v, and no other slot changed a byte
    live = torch.from_numpy(np.nonzero(L > 0)[0])
    named = case["slot"][live].long()
    assert torch.equal(bits(kc[named.cuda()]), bits(qkv[live.cuda(), D:2 * D]))
    assert torch.equal(bits(vc[named.cuda()]), bits(qkv[live.cuda(), 2 * D:]))
    rest = torch.ones(kc.shape[0], dtype=torch.bool)
    rest[named] = False
    assert torch.equal(bits(kc[rest.cuda()]), bits(case["kc"].to(dtype).cuda()[rest.cuda()]))
    assert torch.equal(bits(vc[rest.cuda()]), bits(case["vc"].to(dtype).cuda()[rest.cuda()]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [32, 64])
def test_step_kernel_bitwise_claims(d, dtype):
    """H 3, R 65: NaN / Inf in every slot no row names and other garbage behind the lengths of anc change no bit; row 5 alone is
    row 5 of the batch; two runs agree"""
    case = I.step_case(d, 3, 65)
    o, kc, vc = run_step(case, dtype)
    L, anc = case["lengths"].numpy(), case["anc"]
    used = np.zeros(case["kc"].shape[0], dtype=bool)
    clean = anc.clone()
    for r in range(65):
        n = max(int(L[r]) - 1, 0)
        used[anc[r, :n].numpy()] = True
        assert n == anc.shape[1] or set(anc[r, n:].tolist()) <= {-1, 2 ** 30}    # the garbage the case was built with
        clean[r, n:] = 0
    assert used.sum() >= 300 and (~used).sum() >= 300
    pk, pv = case["kc"].clone(), case["vc"].clone()
    pk[torch.from_numpy(~used)] = float("nan")
    pv[torch.from_numpy(~used)] = float("inf")
    o2, kc2, vc2 = run_step(case, dtype, kc=pk, vc=pv, anc=clean)
    assert torch.equal(bits(o2), bits(o))
    named = case["slot"][torch.from_numpy(np.nonzero(L > 0)[0])].long().cuda()
    assert torch.equal(bits(kc2[named]), bits(kc[named])) and torch.equal(bits(vc2[named]), bits(vc[named]))
    skipped = case["slot"][torch.from_numpy(np.nonzero(L <= 0)[0])].long().cuda()
    assert skipped.numel() and torch.isnan(kc2[skipped]).all() and torch.isinf(vc2[skipped]).all()   # nothing stored there
    assert L[5] == 63
    alone, _, _ = run_step(case, dtype, rows=slice(5, 6))
    assert torch.equal(bits(alone[0]), bits(o[5]))
    again, _, _ = run_step(case, dtype)
    assert torch.equal(bits(again), bits(o))


@functools.lru_cache(maxsize=None)
def causal_ref_rows(kind, d):
    """float64 causal attention of a packed qkv [B, T, 3 H d] (bf16-valued): (qkv, H, out [B, T, H d], max |V|)"""
    if kind == "rising":
        qkv, H = C.rising_causal_qkv(d), C.RISING_H
    else:
        g = torch.Generator().manual_seed(130 + d)
        H = 2
        qkv = torch.randn(1, 130, 3 * H * d, generator=g)
        qkv[..., :H * d] *= 1.5
        qkv[..., 2 * H * d:] += 0.5
        qkv = C.bf16_valued(qkv)
    B, T, _ = qkv.shape
    x = qkv.double().numpy().reshape(B, T, 3, H, d)
    s = np.einsum("bqhd,bkhd->bhqk", x[:, :, 0], x[:, :, 1]) / np.sqrt(d)
    s = np.where(np.triu(np.ones((T, T), dtype=bool), 1)[None, None], -np.inf, s)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    out = np.einsum("bhqk,bkhd->bqhd", p, x[:, :, 2]).reshape(B, T, H * d)
    return qkv, H, out, float(qkv[..., 2 * H * d:].abs().max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [32, 64])
def test_step_kernel_rescales_under_rising_scores(d, dtype):
    """rising_causal_qkv: scores up 0.5 per 32 keys in heads 0 and 2, falling in heads 1 and 3.  A lane holds keys 64 apart, so
    its running maximum is renewed at every key it takes in the rising heads while its earlier keys keep a share of the mass
    (tests/test_transformer_lm.py asserts the profile per 32-key step): a kernel that does not rescale its sum or its output by
    exp(m_old - m_new) misses the bound.  Queries 128 .. 299 of both sequences in one launch over a cache filled by hand."""
    from unispeech_amd import ops
    qkv, H, want, vmax = causal_ref_rows("rising", d)
    B, T, D = qkv.shape[0], qkv.shape[1], H * d
    rng = np.random.default_rng(d)
    perm = rng.permutation(2048)
    tok_slot = perm[:B * T].reshape(B, T)                                        # where token t of sequence b lives
    queries = [(b, t) for b in range(B) for t in range(128, T)]
    own = perm[B * T:B * T + len(queries)]
    kc, vc = torch.zeros(2048, D), torch.zeros(2048, D)
    kc[torch.from_numpy(tok_slot.reshape(-1))] = qkv[..., D:2 * D].reshape(-1, D)
    vc[torch.from_numpy(tok_slot.reshape(-1))] = qkv[..., 2 * D:].reshape(-1, D)
    anc = np.zeros((len(queries), T), dtype=np.int32)
    for r, (b, t) in enumerate(queries):
        anc[r, :t] = tok_slot[b, :t]
    rows = torch.stack([qkv[b, t] for b, t in queries])
    o = ops.attn_step(rows.to(dtype).cuda(), kc.to(dtype).cuda(), vc.to(dtype).cuda(),
                      torch.from_numpy(own.astype(np.int32)).cuda(), torch.from_numpy(anc).cuda(),
                      torch.tensor([t + 1 for _, t in queries], dtype=torch.int32).cuda(), H, T)
    ref = np.stack([want[b, t] for b, t in queries])
    err = np.abs(f64(o) - ref).max()
    print("rising scores", dtype, d, "error", err, "of |V| max", vmax, "=", err / vmax, "bound", kernel_tol(dtype))
    assert np.isfinite(f64(o)).all() and err <= kernel_tol(dtype) * vmax


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [32, 64])
def test_chain_built_step_by_step_is_the_causal_attention(d, dtype):
    """130 tokens, one launch each, every launch reading what the earlier ones stored: the rows of wavlm_attn_causal_fwd on the
    same qkv, each against float64 within its bound"""
    from unispeech_amd import ops
    qkv, H, want, vmax = causal_ref_rows("chain", d)
    T, D = qkv.shape[1], H * d
    x = qkv.to(dtype).cuda()
    perm = torch.from_numpy(np.random.default_rng(d).permutation(256).astype(np.int32)).cuda()
    kc = torch.full((256, D), float("nan"), dtype=dtype, device="cuda")          # a slot is written before it is read
    vc = torch.full((256, D), float("nan"), dtype=dtype, device="cuda")
    rows = []
    for t in range(T):
        anc = perm[:max(t, 1)].view(1, -1).contiguous()
        rows.append(ops.attn_step(x[0, t:t + 1].contiguous(), kc, vc, perm[t:t + 1].contiguous(), anc,
                                  torch.tensor([t + 1], dtype=torch.int32, device="cuda"), H, t + 1))
    o = torch.cat(rows)
    full = ops.attn_causal_fwd(x, H)[0]
    e_step, e_full = np.abs(f64(o) - want[0]).max(), np.abs(f64(full) - want[0]).max()
    print("chain of 130", dtype, d, "step error", e_step / vmax, "causal error", e_full / vmax, "bound", kernel_tol(dtype))
    assert np.isfinite(f64(o)).all() and e_step <= kernel_tol(dtype) * vmax and e_full <= kernel_tol(dtype) * vmax
    assert torch.equal(bits(kc[perm[:T].long()]), bits(x[0, :, D:2 * D])) and torch.isnan(kc[perm[T:].long()]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_step_kernel_refuses_bad_arguments(dtype):
    """-1 before any launch, O and both caches untouched: NULL pointers, pointers or strides that are not 16-byte aligned, a head
    width of 16 or 128, another dtype, ld_anc too short for the longest length, R or H of 0, and two tensors that are one"""
    from unispeech_amd import _lib, ops
    h, p = _lib.lib(), ops.ptr
    d, H, R = 32, 2, 3
    D = H * d
    es = 2 if dtype == torch.bfloat16 else 4
    off = 4 // es                                                               # 4 bytes: off the 16-byte grid
    qkv = torch.ones(R * 3 * D + 64, dtype=dtype, device="cuda")
    kc = torch.full((16 * D + 64,), 7.0, dtype=dtype, device="cuda")
    vc = torch.full((16 * D + 64,), 7.0, dtype=dtype, device="cuda")
    out = torch.full((R * D + 64,), 7.0, dtype=dtype, device="cuda")
    slot = torch.tensor([3, 4, 5, 0], dtype=torch.int32, device="cuda")
    anc = torch.zeros(R * 4 + 4, dtype=torch.int32, device="cuda")
    lengths = torch.tensor([1, 2, 3, 0], dtype=torch.int32, device="cuda")

    def call(q=p(qkv), ldq=3 * D, K=p(kc), V=p(vc), ldk=D, slots=16, s=p(slot), a=p(anc), lda=4, L=p(lengths), mx=3, O=p(out),
             ldo=D, R=R, H=H, hd=d, dt=ops.dt(qkv)):
        return h.wavlm_attn_step(q, ldq, K, V, ldk, slots, s, a, lda, L, mx, O, ldo, R, H, hd, dt, ctypes.c_float(d ** -0.5),
                                 ops.stream())
    for kw in (dict(q=None), dict(K=None), dict(V=None), dict(s=None), dict(a=None), dict(L=None), dict(O=None),
               dict(q=p(qkv, off)), dict(K=p(kc, off)), dict(V=p(vc, off)), dict(O=p(out, off)),
               dict(ldq=3 * D + off), dict(ldk=D + off), dict(ldo=D + off),
               dict(s=p(slot.view(torch.int16), 1)), dict(a=p(anc.view(torch.int16), 1)), dict(L=p(lengths.view(torch.int16), 1)),
               dict(hd=16), dict(hd=128), dict(hd=0), dict(dt=2), dict(dt=-1),
               dict(lda=1), dict(mx=6), dict(mx=0), dict(R=0), dict(H=0), dict(R=-1), dict(slots=0),
               dict(ldq=3 * D - 8), dict(ldk=D - 8), dict(ldo=D - 8),
               dict(O=p(qkv)), dict(K=p(vc)), dict(O=p(kc)), dict(V=p(out)),
               dict(O=p(qkv, 3 * D)), dict(V=p(kc, D))):                        # unequal pointers, overlapping ranges
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (kc == 7.0).all() and (vc == 7.0).all()       # nothing was launched
    assert call() == 0 and call(lda=2, mx=3) == 0                               # ld_anc = max_length - 1 is enough
    torch.cuda.synchronize()
    o = out[:R * D].view(R, D).float()                                          # own v = 1, slot 0 holds 7
    assert (o[0] == 1.0).all() and (o[1:] >= 1.0).all() and (o[1:] <= 7.0).all() and (out[R * D:] == 7.0).all()
    assert (kc[3 * D:6 * D] == 1.0).all() and (kc[:3 * D] == 7.0).all() and (kc[6 * D:] == 7.0).all()
    # what the device finds: a length above max_length, a slot or a read ancestor outside the cache -- NaN, nothing stored
    vc.fill_(7.0)
    kc.fill_(7.0)
    bad_slot = torch.tensor([3, 16, -1, 0], dtype=torch.int32, device="cuda")
    bad_anc = torch.tensor([99, 99, 99, 99, 16, 99, 99, 99, 0, -1, 99, 99, 0, 0, 0, 0], dtype=torch.int32, device="cuda")
    assert call(s=p(bad_slot)) == 0
    torch.cuda.synchronize()
    o = out[:R * D].view(R, D).float()
    assert (o[0] == 1.0).all() and torch.isnan(o[1:]).all() and (kc[4 * D:] == 7.0).all() and (vc[4 * D:] == 7.0).all()
    vc.fill_(7.0)
    kc.fill_(7.0)
    assert call(a=p(bad_anc)) == 0
    torch.cuda.synchronize()
    o = out[:R * D].view(R, D).float()
    assert (o[0] == 1.0).all() and torch.isnan(o[1:]).all()
    assert (kc == 7.0).sum() == kc.numel() - D and (kc[3 * D:4 * D] == 1.0).all()    # only row 0 (length 1) stored
    kc.fill_(7.0)
    assert call(mx=2) == 0                                                       # row 2 is longer than the promised maximum
    torch.cuda.synchronize()
    o = out[:R * D].view(R, D).float()
    assert torch.isfinite(o[:2]).all() and torch.isnan(o[2]).all()
    assert (kc[3 * D:5 * D] == 1.0).all() and (kc[5 * D:] == 7.0).all() and (kc[:3 * D] == 7.0).all()


# ---------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def gi():
    return load_golden("transformer_lm_incremental.npz")


def mode_bound(g, name, dtype):
    return (HEAD_TOL if dtype == torch.float32 else 2 * float(g[name + "/e_ref"])) * float(g[name + "/max"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(C.MODELS))
def test_model_chains_against_the_fixtures(gi, name, dtype):
    """models A, B and C, every sentence walked one word per extend(): full rows against transformer_lm_incremental.npz, target
    entries against transformer_lm.npz"""
    g = load_golden("transformer_lm.npz")
    store = C.build(name, dtype, "cuda").incremental(chunk=16)                   # 46 states: the caches grow twice
    worst = worst_t = 0.0
    for i, s in enumerate(C.sentences()):
        rows = store.logprob_rows(I.walk_chain(store, s))
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (len(s) + 1, C.VOCAB) and rows.is_cuda
        rows = f64(rows)
        assert np.abs(np.exp(rows).sum(1) - 1).max() <= 1e-3                    # the lse is the fused kernel's, the logits a GEMM's
        if i in I.GOLDEN_SENTENCES:
            worst = max(worst, np.abs(rows - gi["%s/rows_%d" % (name, i)]).max())
        want = g[name + "/logprobs"][i, :len(s) + 1]
        got = np.array([rows[t, w] for t, w in enumerate(s + [C.EOS])])
        fin = np.isfinite(want)
        worst_t = max(worst_t, np.abs(got[fin] - want[fin]).max())
    assert len(store) == 1 + sum(len(s) for s in C.sentences()) and store.cap == 64
    print("model", name, dtype, "full rows: error %.3e (bound %.3e); target entries: %.3e (bound %.3e)"
          % (worst, mode_bound(gi, name, dtype), worst_t, mode_bound(g, name, dtype)))
    assert worst <= mode_bound(gi, name, dtype) and worst_t <= mode_bound(g, name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(C.WIDE_MODELS))
def test_wide_model_walks_200_words(name, dtype):
    """models W and X (heads 64 and 32 wide, V 5003) over the 200-word sentence of wide_sentences(): depth crosses 128, the
    GEMMs run at M = 1; against tests/golden/transformer_lm_wide.npz"""
    gw = load_golden("transformer_lm_wide.npz")
    s = C.wide_sentences()[5]
    store = C.build_wide(name, dtype, "cuda").incremental()
    states = I.walk_chain(store, s)
    tgt = s + [C.EOS]
    lp = f64(store.logprob_rows(states))[np.arange(201), tgt]
    some = f64(store.logprob_rows(states[100:103], [tgt[100], 4, C.WIDE_VOCAB - 1]))
    assert some.shape == (3, 3) and abs(some[0, 0] - lp[100]) <= 1e-4           # three gathered columns: another GEMM shape
    want = gw[name + "/logprobs"][5]
    assert want.shape == (201,) and np.isfinite(want).all()
    err = np.abs(lp - want).max() / float(gw[name + "/max"])
    bound = HEAD_TOL if dtype == torch.float32 else 2 * float(gw[name + "/e_ref"])
    print("model", name, dtype, "200 words one at a time: error %.3e of the max magnitude (bound %.3e)" % (err, bound))
    assert err <= bound


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(C.MODELS))
def test_model_tree_against_score(gi, name, dtype):
    """the branching tree of the CPU test, several rows per extend() where the tree allows it, against TransformerLM.score of the
    two full sentences and against the float64 rows"""
    from unispeech_amd.transformer_lm import _forward64
    m = C.build(name, dtype, "cuda")
    store = m.incremental()
    walks = I.walk_tree(store)
    lp, _ = m.score(I.tree_sentences())
    bound = mode_bound(gi, name, dtype)
    m64 = C.build(name)
    for k, (states, s) in enumerate(zip(walks, I.tree_sentences())):
        rows = f64(store.logprob_rows(states))
        got = np.array([rows[t, w] for t, w in enumerate(s + [C.EOS])])
        e_score = np.abs(got - lp[k, :len(s) + 1].numpy()).max()
        with torch.no_grad():
            e_64 = np.abs(rows - _forward64(m64, s).numpy()).max()
        print("model", name, dtype, "tree sentence", k, "against score %.3e, against float64 %.3e (bound %.3e)" % (e_score, e_64, bound))
        assert e_score <= bound and e_64 <= bound
    # both continuations of the prefix in one call, then one more level for both: the same rows within the bound
    single = np.concatenate([f64(store.logprob_rows(walks[0][4:6])), f64(store.logprob_rows(walks[1][4:6]))])
    store.reset()
    st = I.walk_chain(store, I.TREE_PREFIX)
    a, b = store.extend([st[-1], st[-1]], [I.TREE_OLD[0], I.TREE_NEW[0]])
    a2, b2 = store.extend([a, b], [I.TREE_OLD[1], I.TREE_NEW[1]])
    batched = f64(store.logprob_rows([a, a2, b, b2]))
    assert np.abs(batched - single).max() <= bound


def test_device_store_refuses_a_depth_beyond_max_target_positions():
    store = C.build("B", torch.float32, "cuda").incremental(chunk=64)            # max_target_positions 64
    st = I.walk_chain(store, [5] * 63)
    assert len(store) == 64 and store.cap == 64
    with pytest.raises(ValueError, match="max_target_positions"):
        store.extend([st[-1]], [5])
    with pytest.raises(ValueError, match="dictionary"):
        store.extend([0], [C.VOCAB])
    assert len(store) == 64 and store.extend([st[3]], [6]) == [64] and store.cap == 128


# --------------------------------------------------------------------------------------------------------- the search
def run_fused(dtype):
    from unispeech_amd import ctc_lexicon as X
    x, il, d, lexicon, opts, lm_dict = I.search_case(C.build("A", dtype, "cuda"))
    stats = {}
    got = X.fused_lexicon_decode(x.cuda(), il, d, lexicon, lexicon.lm, normalized=True, stats=stats, **opts)
    return got, stats, opts


def test_fused_search_fp32_mode_returns_the_float64_hypotheses(gi):
    """fp32 mode: words and tokens of every returned hypothesis of both utterances equal the float64 run's, scores within
    tol = lm_weight x (longest word count + 1) x HEAD_TOL x max |log-prob|.  No utterance is excused: the float64 run's smallest
    margin between unequal scores exceeds 2 tol (asserted here again; tests/test_lm_incremental.py derives it)."""
    want, margins, mx, states, _ = I.search_reference()
    got, stats, opts = run_fused(torch.float32)
    tol = I.search_tol(want, HEAD_TOL * mx, opts["lm_weight"])
    assert min(margins) > 2 * tol
    assert stats["states"] == states and all(c <= 13 for c in stats["calls"])
    worst = 0.0
    for gu, wu in zip(got, want):
        assert [(h[0], h[1]) for h in gu] == [(h[0], h[1]) for h in wu]
        worst = max(worst, max(abs(a[2] - b[2]) for a, b in zip(gu, wu)))
    print("fused search fp32 mode: largest score difference %.3e (tol %.3e, smallest margin %.3e)" % (worst, tol, min(margins)))
    assert worst <= tol


def test_fused_search_bf16_mode_stays_near_the_float64_optimum(gi):
    """bf16 mode, tol with 2 e_ref in place of HEAD_TOL: the float64 objective of each returned 1-best (its score in the float64
    run's whole final beam) equals the returned score within tol and lies within 2 tol of the float64 optimum.  The winner's
    identity is not asserted: the float64 margin is smaller than twice this tolerance."""
    want, margins, mx, _, whole = I.search_reference()
    got, stats, opts = run_fused(torch.bfloat16)
    tol = I.search_tol(want, 2 * float(gi["A/e_ref"]) * mx, opts["lm_weight"])
    for b, (gu, wu) in enumerate(zip(got, want)):
        words, tokens, score = gu[0]
        key = (tuple(words), tuple(tokens))
        assert key in whole[b], "the bf16 winner is not in the float64 run's final beam"
        obj = whole[b][key]
        print("fused search bf16 mode, utterance %d: returned %.4f, float64 objective %.4f, float64 optimum %.4f (tol %.4f)"
              % (b, score, obj, wu[0][2], tol))
        assert abs(obj - score) <= tol and wu[0][2] - obj <= 2 * tol
        assert [h[2] for h in gu] == sorted((h[2] for h in gu), reverse=True)


def test_fused_command_line_is_the_function(tmp_path, capsys):
    """`ctc_lexicon decode --fuse-lm` on the tiny CTC checkpoint of tests/test_ctc_lexicon_gpu.py with model A written as a
    checkpoint prints what fused_lexicon_decode returns on the same emissions with the same model (the same launches): a check
    of the command line's plumbing only -- what the search returns is checked by the two search tests above"""
    from test_ctc_lexicon_gpu import _e2e_logits, _e2e_setup
    from unispeech_amd import ctc, ctc_lexicon as X
    d, lexicon0, loaded, wavs, labels, arpa = _e2e_setup(tmp_path)
    words = [w for w in lexicon0.words if w != "<unk>"][:C.VOCAB - 4]
    (tmp_path / "lm.dict.txt").write_text("".join("%s 1\n" % w for w in words + ["pad%d" % i for i in range(C.VOCAB - 4 - len(words))]))
    torch.save({"cfg": dict(C.MODELS["A"]), "model": C.build("A").state_dict()}, str(tmp_path / "lm.pt"))
    lm_dict = ctc.LetterDictionary.load(str(tmp_path / "lm.dict.txt"))
    flags = ["--lexicon", str(tmp_path / "lex.txt"), "--beam", "5", "--beam-size-token", "4", "--beam-threshold", "inf",
             "--lm-weight", "0.5", "--word-score", "-0.5", "--sil-weight", "-0.25", "--nbest", "3",
             "--fuse-lm", str(tmp_path / "lm.pt"), "--fuse-dict", str(tmp_path / "lm.dict.txt")]
    assert X.main(["decode", str(tmp_path / "ck.pt"), str(tmp_path / "dict.ltr.txt")] + wavs + flags) == 0
    out = capsys.readouterr().out.splitlines()
    lw, spellings = X.read_lexicon(str(tmp_path / "lex.txt"), d)
    lexicon = X.Lexicon(lw, spellings, d, X.NeuralWordLM(C.build("A", torch.float32, "cuda"), lm_dict, lw))
    single, _, _ = _e2e_logits(loaded, wavs)
    k = 0
    for x in single:
        hyps = X.fused_lexicon_decode(x, None, d, lexicon, lexicon.lm, beam=5, beam_size_token=4, beam_threshold=math.inf,
                                      lm_weight=0.5, word_score=-0.5, sil_weight=-0.25, nbest=3)[0]
        assert hyps
        for wds, _, sc in hyps:
            score, text = out[k].split("\t")
            assert text == " ".join(wds) and abs(float(score) - sc) <= 1e-4
            k += 1
    assert k == len(out)
    with pytest.raises(SystemExit):
        X.main(["decode", str(tmp_path / "ck.pt"), str(tmp_path / "dict.ltr.txt")] + wavs + flags + ["--lm", arpa])
    capsys.readouterr()
