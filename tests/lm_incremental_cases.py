"""Shared by tests/test_lm_incremental.py and tests/test_lm_incremental_gpu.py: the branching tree of word histories, the built
cases of wavlm_attn_step (csrc/lm_step.hip) with their float64 results, and the fused-search case."""
import functools

import numpy as np
import torch

import transformer_lm_cases as C

HEAD_TOL = 5e-4                        # tests/test_transformer_lm_gpu.py: the fp32-mode bound of a head, of the max magnitude
GOLDEN_SENTENCES = (1, 2, 3)           # tools/gen_transformer_lm_incremental_golden.py SENTENCES


# ------------------------------------------------------------------------------------------------------------ the tree
TREE_PREFIX, TREE_OLD, TREE_NEW = [5, 25, 77], [40, 9, 61], [12, 88]


def tree_sentences():
    """the two full sentences of the tree: a shared prefix of three words, then the older and the newer continuation"""
    return [TREE_PREFIX + TREE_OLD, TREE_PREFIX + TREE_NEW]


def walk_tree(store):
    """shared prefix, the first word of the older branch, the whole newer branch, then the rest of the older one -- so the older
    branch is extended after states that are not its ancestors took the slots behind it.  -> per sentence its state ids in
    position order, the start state first"""
    st = [store.start()]
    for w in TREE_PREFIX:
        st += store.extend([st[-1]], [w])
    old = store.extend([st[-1]], TREE_OLD[:1])
    new = []
    for w in TREE_NEW:
        new += store.extend([(new or st)[-1]], [w])
    for w in TREE_OLD[1:]:
        old += store.extend([old[-1]], [w])
    return [st + old, st + new]


def walk_chain(store, words):
    """the states of [eos], [eos, w_1], ... one extend() per word"""
    st = [store.start()]
    for w in words:
        st += store.extend([st[-1]], [w])
    return st


# ------------------------------------------------------------------------------------------- wavlm_attn_step: built cases
STEP_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 192, 193, 300, 0, -3)
# 64 keys per pass of a wave (key j on lane j % 64): 63 / 64 / 65 and 127 / 128 / 129 are the neighbours of its boundaries, 192 /
# 193 those of the fourth pass; 32 and 33 the last lane a 32-wide head's output leaves from


def bf16_valued(t):
    return t.to(torch.bfloat16).float()


def step_tree(seed, n_nodes, depth_cap=299):
    """a random tree over n_nodes nodes with shared prefixes: node 0 is a root, node i's parent is a random earlier node (or, one
    time in eight, none: another root) whose depth is below depth_cap; one long chain is forced so that depth_cap is reached.
    -> (parent [n], depth [n])"""
    rng = np.random.default_rng(seed)
    parent, depth = np.full(n_nodes, -1, dtype=np.int64), np.zeros(n_nodes, dtype=np.int64)
    for i in range(1, n_nodes):
        if i <= depth_cap:
            p = i - 1                                            # the spine: depths 0 .. depth_cap
        elif rng.integers(8) == 0:
            continue
        else:
            p = int(rng.integers(0, i))
            while depth[p] >= depth_cap:
                p = int(parent[p])
        parent[i], depth[i] = p, depth[p] + 1
    return parent, depth


@functools.lru_cache(maxsize=None)
def step_case(d, H, R, seed=0):
    """One launch of wavlm_attn_step over a filled cache, bf16-valued operands.  A tree of 700 nodes lives in a shuffled slot
    numbering of a cache of 1024 slots; the R rows of the launch are new children of nodes chosen so that their lengths run
    through STEP_LENGTHS (cyclically), 0 and negative among them.  -> dict of fp32 / int32 CPU tensors:
      kc, vc [1024, H d]   the cache before the launch (slots of the tree filled, the others zero)
      qkv [R, 3 H d], slot [R], anc [R, ld_anc], lengths [R], max_length
      out float64 [R, H d] the result, vmax = max |V| over everything a row attends"""
    n_nodes, slots = 700, 1024
    g = torch.Generator().manual_seed(1000 * d + 10 * H + R + seed)
    rng = np.random.default_rng(7 + seed)
    parent, depth = step_tree(11 + seed, n_nodes)
    perm = rng.permutation(slots)
    node_slot, free = perm[:n_nodes], perm[n_nodes:]
    D = H * d
    kc, vc = torch.zeros(slots, D), torch.zeros(slots, D)
    kc[node_slot] = bf16_valued(torch.randn(n_nodes, D, generator=g))
    vc[node_slot] = bf16_valued(torch.randn(n_nodes, D, generator=g) + 0.5)
    qkv = torch.randn(R, 3 * D, generator=g)
    qkv[:, :D] *= 1.5
    qkv[:, 2 * D:] += 0.5
    qkv = bf16_valued(qkv)
    lengths = np.array([STEP_LENGTHS[r % len(STEP_LENGTHS)] for r in range(R)], dtype=np.int64)
    if R == 1:
        lengths[0] = 130
    max_length = int(max(lengths.max(), 1))
    ld_anc = max_length + 3                                        # wider than needed: the tail holds garbage
    anc = np.where(rng.integers(2, size=(R, ld_anc)) == 0, -1, 2 ** 30).astype(np.int64)
    assert R <= len(free)
    out = np.zeros((R, D))
    for r in range(R):
        L = int(lengths[r])
        if L <= 0:
            continue
        chain = []
        if L > 1:
            cands = np.nonzero(depth == L - 2)[0]                 # the parent's depth: the row is token L - 1
            p = int(cands[rng.integers(len(cands))])
            while p >= 0:
                chain.append(p)
                p = int(parent[p])
            chain.reverse()
        anc[r, :L - 1] = node_slot[chain]
        q, k, v = (qkv[r, i * D:(i + 1) * D].double().numpy().reshape(H, d) for i in range(3))
        K = np.concatenate([kc[node_slot[chain]].double().numpy().reshape(-1, H, d), k[None]])
        V = np.concatenate([vc[node_slot[chain]].double().numpy().reshape(-1, H, d), v[None]])
        s = np.einsum("hd,thd->ht", q, K) / np.sqrt(d)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        out[r] = np.einsum("ht,thd->hd", p, V).reshape(D)
    vmax = float(max(vc.abs().max(), qkv[:, 2 * D:].abs().max()))
    return dict(kc=kc, vc=vc, qkv=qkv, slot=torch.from_numpy(free[:R].astype(np.int32)), anc=torch.from_numpy(anc.astype(np.int32)),
                lengths=torch.from_numpy(lengths.astype(np.int32)), max_length=max_length, out=out, vmax=vmax, H=H, d=d)


# ------------------------------------------------------------------------------------------------------- the fused search
SEARCH_NBEST = 4
# The emissions of rescoring() lie on a grid of 1 / 64, so acoustic sums tie exactly and the LM terms, added in another order,
# leave differences of 1e-15 between candidates that are equal on paper: decisions no arithmetic can be asked to reproduce.  With
# beam 63 and lm_weight 1 the smallest margin between unequal scores of the float64 run is 1.8e-15.  So the search case keeps
# rescoring()'s geometry, lexicon, dictionaries and options but draws continuous emissions (log-softmax of 3 N(0, 1), this seed) and
# runs with beam 10 and lm_weight 0.2: of the seeds 1000 .. 1199 this is the one whose float64 run is decided by the widest margin
# (0.037 and 0.048 against a tolerance of 0.0045), found from float64 alone.
SEARCH_SEED = 1127
SEARCH_OPTS = dict(beam=10, lm_weight=0.2)


@functools.lru_cache(maxsize=None)
def search_emissions():
    x0 = C.rescoring()[0]
    z = 3.0 * np.random.default_rng(SEARCH_SEED).standard_normal(tuple(x0.shape))
    return torch.log_softmax(torch.from_numpy(z), -1).float()                # passed as normalized


def search_case(lm_or_store):
    """the rescoring() case of tests/transformer_lm_cases.py (T 12, B 2, C 12, lexicon `mid`, LM dictionary of 100) with
    search_emissions(), a NeuralWordLM over `lm_or_store` in the lexicon, SEARCH_OPTS and 4-best: (emissions, input lengths,
    dictionary, Lexicon, options, the LM's dictionary)"""
    import ctc_lexicon_cases as L
    from unispeech_amd import ctc_lexicon as X
    _, il, d, _, opts, lm_dict = C.rescoring()
    words, spellings = X.read_lexicon(L.lexicon_path("mid"), d)
    lexicon = X.Lexicon(words, spellings, d, X.NeuralWordLM(lm_or_store, lm_dict, words))
    return search_emissions(), il, d, lexicon, dict(opts, nbest=SEARCH_NBEST, **SEARCH_OPTS), lm_dict


@functools.lru_cache(maxsize=None)
def search_reference():
    """the float64 run of the fused search on model A: (hyps as fused_lexicon_decode returns them, the smallest margin among the
    decisions between unequal scores per utterance, max |log-prob| over the finite entries of every LM row the run read,
    the states it evaluated per utterance, and per utterance {(words, tokens): score} of the same search's whole final beam)"""
    from unispeech_amd import ctc, ctc_lexicon as X
    from unispeech_amd.transformer_lm import incremental_reference
    x, il, d, lexicon, opts, _ = search_case(incremental_reference(C.build("A")))
    lm, hyps, margins, mx, states, whole = lexicon.lm, [], [], 0.0, [], []
    for b in range(x.shape[1]):
        lm.empty_cache()
        n0 = lm.evaluated
        res = X.lexicon_beam_search_reference(x[:, b:b + 1], [il[b]], lexicon, d.bos(), ctc.silence_token(d), normalized=True,
                                              prepare=lm.prepare, unequal_margins=margins, **opts)[0][0]
        hyps.append([([lexicon.words[w] for w in wds], toks, sc) for wds, toks, sc in res])
        states.append(lm.evaluated - n0)
        res = X.lexicon_beam_search_reference(x[:, b:b + 1], [il[b]], lexicon, d.bos(), ctc.silence_token(d), normalized=True,
                                              **dict(opts, nbest=opts["beam"]))[0][0]
        whole.append({(tuple(lexicon.words[w] for w in wds), tuple(toks)): sc for wds, toks, sc in res})
        for row in lm._rows.values():
            mx = max(mx, float(np.abs(row[np.isfinite(row)]).max()))
    return hyps, margins, mx, states, whole


def search_tol(hyps, per_token, lm_weight):
    """lm_weight x (longest word count + 1) x the bound on one LM entry"""
    longest = max(len(h[0]) for utt in hyps for h in utt)
    return lm_weight * (longest + 1) * per_token
