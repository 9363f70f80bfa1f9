"""Shared by tests/test_seq2seq_fusion.py, tests/test_seq2seq_fusion_gpu.py and tools/gen_seq2seq_fusion_golden.py: the language
models fused into the two seq2seq models of tests/seq2seq_cases.py, the option sets of tests/golden/seq2seq_fusion.npz, and the
seeded builder of the cases of wavlm_beam_step_fused.

  seq2seq model A  +  an LM of configuration transformer_lm_cases.MODELS["B"] (post-LN, GELU, learned positions, shared embedding)
  seq2seq model B  +  an LM of configuration transformer_lm_cases.MODELS["A"] (pre-LN + final norm, sinusoidal positions)
both at the seq2seq dictionary's 12 entries, filled by transformer_lm_cases.fill_state_dict(seed) (no weights are stored).
Option sets, each at beams 1 and 5 with max_len_b 12:
  F   lm_weight 0.7                  models A and B
  FN  lm_weight 0.7, n = 3           models A and B
  N   no LM, n = 2                   model A (model B's beam-5 margin under it is below 1e-3)"""
import functools
import math

import numpy as np
import torch

import seq2seq_cases as C
import transformer_lm_cases as LC

LM_CONFIG = {"A": "B", "B": "A"}       # seq2seq model -> configuration of its LM
LM_SEEDS = {"A": 101, "B": 102}        # chosen by tools/gen_seq2seq_fusion_golden.py's assertions (A = 103: FN's beam-5 score
#                                        gap is 2e-4; 100, 102 and 104 miss a margin or a gap as well)
LM_WEIGHT = 0.7
SETS = {
    "F": dict(lm=True, lm_weight=LM_WEIGHT, no_repeat_ngram_size=0, models=("A", "B")),
    "FN": dict(lm=True, lm_weight=LM_WEIGHT, no_repeat_ngram_size=3, models=("A", "B")),
    "N": dict(lm=False, lm_weight=1.0, no_repeat_ngram_size=2, models=("A",)),
}
GOLDEN = "seq2seq_fusion.npz"


def runs():
    """(model, set, beam) of every stored run"""
    return [(m, s, k) for s, o in SETS.items() for m in o["models"] for k in C.BEAMS]


def lm_options(name):
    return dict(LC.MODELS[LM_CONFIG[name]])


def build_lm(name, dtype=torch.float32, device=None):
    """this package's LM for seq2seq model `name` with the filled weights -- built anew at every call"""
    from unispeech_amd.transformer_lm import TransformerLM
    opts = lm_options(name)
    m = TransformerLM(opts, C.VOCAB, pad=C.PAD, eos=C.EOS, unk=C.UNK)
    m.load_state_dict(LC.fill_state_dict(m.state_dict(), LM_SEEDS[name], opts.get("share_decoder_input_output_embed", False)),
                      strict=False)
    if device is not None:
        m = m.to(device)
    return m.to(dtype)


def repeats(tokens, n):
    """does the hypothesis (without its bos) hold an n-gram twice?  The blocker looks at the row from the bos on."""
    h = [C.EOS] + [int(t) for t in tokens]
    grams = [tuple(h[i:i + n]) for i in range(len(h) - n + 1)]
    return len(set(grams)) != len(grams)


# ------------------------------------------------------------------------------------- wavlm_beam_step_fused: built cases
FUSED_V = (32, 2049, 10001)
FUSED_WIDTHS = (1, 5, 32)
FUSED_N = (0, 1, 2, 3, 4)
FUSED_WEIGHTS = (None, 0.0, 0.7, 2.0)
ALPHABET = (4, 5, 6)                   # histories over three symbols: bans are frequent
LONG_STEP = 300                        # a history longer than one pass of the kernel's 256 threads


def fused_steps(n):
    """steps 0, n - 2, n - 1 and 11 (those that are >= 0), and n + 1: the first steps at which a ban can bite"""
    return sorted({s for s in (0, n - 2, n - 1, n + 1, 11) if s >= 0})


def ban_possible(n, step):
    """can the blocker ban a token that is not -inf already?  The bos differs from every symbol of ALPHABET, so an n-gram that
    begins at position 0 never recurs: the first window that can match begins at 1 and must end before the tail's last token --
    step >= n for n >= 2.  n = 1 bans the history itself: at step 0 that is the bos (= eos, which min_len holds at -inf)."""
    return n > 0 and step >= max(n, 1)


def fused_cases():
    """(V, beam, n, lm_weight, step): n x weights x steps at V 2049 beam 5, every V x beam at (n 3, weight 0.7, step 11) and
    (n 0, weight 0.7, step 11), and the long case"""
    out = [(2049, 5, n, w, s) for n in FUSED_N for w in FUSED_WEIGHTS for s in fused_steps(n)]
    out += [(V, beam, n, 0.7, 11) for V in FUSED_V for beam in FUSED_WIDTHS for n in (0, 3) if (V, beam) != (2049, 5)]
    out.append((2049, 5, 3, 0.7, LONG_STEP))
    return out


@functools.lru_cache(maxsize=None)
def fused_case(V, beam, n, lm_weight, step, seed=0, ties=False):
    """one call of wavlm_beam_step_fused over B = 3 sentences on a consistent state: sentence 1 finished earlier; at step > 0
    full beams, one row of sentence 2 at -inf where beam > 1; row r's position j sits in slot j * R + r and tree_token holds
    the histories (bos, then symbols of ALPHABET; the last one is the row's token).  Two model logits at -inf; with an LM:
    one LM entry at -inf (a token the model likes: with lm_weight 0 that is 0 * -inf), one NaN LM row where beam > 2.
    Float64 scores of neighbours among the best 2 beam + 1 differ by more than BEAM_GAP (1 + |lm_weight|), and with n > 0 and
    step >= n - 1 some row's unbanned best token is banned: the seed is advanced until both hold.  ties: integer logits."""
    from unispeech_amd.seq2seq import beam_step_reference
    B, R = 3, 3 * beam
    max_len = max(12, step + 1)
    w = 0.0 if lm_weight is None else float(lm_weight)
    for attempt in range(400):
        g = torch.Generator().manual_seed(9000 + 1000 * seed + 17 * V + beam + 31 * n + 7 * step + 100003 * attempt)
        if ties:
            logits = torch.randint(0, 3, (R, V), generator=g).float()
            lm = torch.randint(0, 3, (R, V), generator=g).float()
            cum = -torch.randint(0, 3, (R,), generator=g).float()
        else:
            logits = 3.0 * torch.randn(R, V, generator=g)
            lm = 2.0 * torch.randn(R, V, generator=g)
            cum = -5.0 * torch.rand(R, generator=g)
        hist = torch.tensor(ALPHABET)[torch.randint(0, len(ALPHABET), (R, step + 1), generator=g)]
        hist[:, 0] = C.EOS
        for r in range(R):                                            # the alphabet is what the model likes: bans matter
            logits[r, list(ALPHABET)] += 6.0 if not ties else 3.0
        if step == 0:
            cum = torch.zeros(R)
            n_live, n_fin = [1, 0, 1], [0, beam, 0]
        else:
            n_live, n_fin = [beam, 0, beam], [0, beam, min(2, beam - 1)]
            if beam > 1 and not ties:
                cum[2 * beam + 1] = -math.inf
        if not ties:
            logits[0, 0] = logits[0, V - 1] = -math.inf
            lm[0, ALPHABET[1]] = -math.inf
            if beam > 2 and step > 0:
                lm[2 * beam + 2, 7] = math.nan
        case = dict(logits=logits, lm=None if lm_weight is None else lm, lm_weight=w, n=n, cum=cum, n_live=n_live, n_fin=n_fin,
                    step=step, max_len=max_len, min_len=1, unk_penalty=0.5, V=V, beam=beam, hist=hist, ties=ties)
        exp = fused_expected(case)
        if ties:                                                      # equal entries of one row tie exactly in every precision;
            gaps = [a - c for e in exp if e is not None               # two rows' scores must not come close without being equal
                    for (a, _), (c, _) in zip(e["candidates"][:-1], e["candidates"][1:]) if a > -math.inf and c > -math.inf]
            if all(g == 0.0 or g > C.BEAM_GAP * (1 + abs(w)) for g in gaps) and any(g == 0.0 for g in gaps):
                return case
            continue
        ok, sensitive = True, False
        for b in range(B):
            if n_live[b] == 0:
                continue
            rows = slice(b * beam, b * beam + n_live[b])
            r = beam_step_reference(logits[rows].double(), cum[rows].double(), step, n_fin[b], full=True, **fused_options(case, b))
            s = [v for v, _ in r["all"][:2 * beam + 1] if v > -math.inf]
            if any(a - c <= C.BEAM_GAP * (1 + abs(w)) for a, c in zip(s[:-1], s[1:])):
                ok = False
            if n > 0:
                free = beam_step_reference(logits[rows].double(), cum[rows].double(), step, n_fin[b], full=True,
                                           **dict(fused_options(case, b), no_repeat_ngram_size=0, history=None))
                best = {}
                for v, i in free["all"]:
                    if v > -math.inf:
                        best.setdefault(i // V, i % V)
                sensitive = sensitive or any(t in exp[b]["banned"][k] for k, t in best.items())
        if ok and (sensitive or not ban_possible(n, step)):
            case["sensitive"] = sensitive
            return case
    raise AssertionError("no seed gives a separated, sensitive case for V=%d beam=%d n=%d w=%r step=%d" % (V, beam, n, lm_weight, step))


def fused_options(case, b):
    beam, nl = case["beam"], case["n_live"][b]
    rows = slice(b * beam, b * beam + nl)
    o = dict(beam=beam, max_len=case["max_len"], min_len=case["min_len"], pad=C.PAD, unk=C.UNK, eos=C.EOS,
             unk_penalty=case["unk_penalty"], temperature=1.0, len_penalty=1.0, normalize_scores=True,
             no_repeat_ngram_size=case["n"], history=[h.tolist() for h in case["hist"][rows]] if case["n"] > 0 else None)
    if case["lm"] is not None:
        o.update(lm_logits=case["lm"][rows].double(), lm_weight=case["lm_weight"])
    return o


def fused_expected(case):
    """per sentence: None where nothing lives, else beam_step_reference's float64 result"""
    from unispeech_amd.seq2seq import beam_step_reference
    beam, out = case["beam"], []
    for b, nl in enumerate(case["n_live"]):
        if nl == 0:
            out.append(None)
            continue
        rows = slice(b * beam, b * beam + nl)
        out.append(beam_step_reference(case["logits"][rows].double(), case["cum"][rows].double(), case["step"], case["n_fin"][b],
                                       **fused_options(case, b)))
    return out


def fused_banned(case):
    """bool [R, V]: the entries of the live rows the blocker bans"""
    R, V, beam = case["logits"].shape[0], case["V"], case["beam"]
    out = np.zeros((R, V), dtype=bool)
    if case["n"] > 0:
        from unispeech_amd.seq2seq import ngram_banned
        for b, nl in enumerate(case["n_live"]):
            for k in range(nl):
                for t in ngram_banned(case["hist"][b * beam + k].tolist(), case["step"], case["n"]):
                    out[b * beam + k, t] = True
    return out
