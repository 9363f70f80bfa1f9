"""The plain references that the `gumbel_vq` and `sampled_negatives` groups of tests/gpu_checks.py compare the kernels with,
against the oracle (which tests/test_oracle_vs_golden.py / test_oracle_vs_reference.py pin to the reference project): a mistake
in a new reference must not be one the kernel shares.  CPU only, fp32, the oracle's own random draws."""
import pytest
import torch

from oracle import wavlm_oracle as O
from unispeech_amd import functional as F

import gpu_checks as K


def _oracle_vq(logits, vars_, G, V, tau, training):
    """oracle.gumbel_vq on given logits: an identity weight projection (exact in fp32: every other product is a zero)"""
    n, GV = logits.shape
    sd = {"q.weight_proj.weight": torch.eye(GV), "q.weight_proj.bias": torch.zeros(GV), "q.vars": vars_}
    return O.gumbel_vq(sd, "q.", logits.view(1, n, GV), G, V, tau, training)


@pytest.mark.parametrize("G,V,n", [(2, 20, 45), (2, 320, 301)])
@pytest.mark.parametrize("training", [False, True])
def test_ref_gumbel_vq_matches_oracle(G, V, n, training):
    logits = K.gen(n, G * V, seed=11, scale=3.0)
    vars_ = K.gen(1, G * V, 6, seed=12)
    vars_[0, :, 0] = torch.arange(G * V, dtype=torch.float32)       # component 0 names the code: indices can be read off x
    torch.manual_seed(1234)
    noise = F.host_gumbel_noise(n * G, V) if training else None
    torch.manual_seed(1234)
    want = _oracle_vq(logits, vars_, G, V, 0.7, training)
    x, prob, code, idx, y_soft = K.ref_gumbel_vq(logits, vars_, G, V, 0.7, training, noise)
    got_idx = idx + torch.arange(G) * V
    want_idx = want["x"].view(n, G, 6)[..., 0].round().long()
    assert torch.equal(got_idx, want_idx)
    torch.testing.assert_close(x, want["x"].view(n, -1), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(prob, want["prob_perplexity"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(code, want["code_perplexity"], rtol=1e-6, atol=1e-6)
    if training:
        torch.manual_seed(1234)
        ys = torch.nn.functional.gumbel_softmax(logits.view(n * G, V), tau=0.7, hard=False)
        torch.testing.assert_close(y_soft, ys, rtol=1e-6, atol=1e-6)


def test_ref_gumbel_vq_gradients_match_oracle():
    """straight-through + diversity gradients of the reference == the oracle's on the same draws (the oracle's
    F.gumbel_softmax runs on lg.float(): agreement to fp32 rounding)"""
    G, V, n = 2, 20, 33
    logits = K.gen(n, G * V, seed=21, scale=3.0).double()
    vars_ = K.gen(1, G * V, 4, seed=22).double()
    w = K.gen(n, G * 4, seed=23).double()
    grads = []
    for which in ("ref", "oracle"):
        lg, vs = logits.clone().requires_grad_(True), vars_.clone().requires_grad_(True)
        torch.manual_seed(99)
        if which == "ref":
            x, prob, _, _, _ = K.ref_gumbel_vq(lg, vs, G, V, 2.0, True, F.host_gumbel_noise(n * G, V).double())
        else:
            sd = {"q.weight_proj.weight": torch.eye(G * V, dtype=torch.float64), "q.weight_proj.bias": torch.zeros(G * V, dtype=torch.float64),
                  "q.vars": vs}
            r = O.gumbel_vq(sd, "q.", lg.view(1, n, G * V), G, V, 2.0, True)
            x, prob = r["x"].view(n, -1), r["prob_perplexity"]
        grads.append(torch.autograd.grad((x * w).sum() - 0.1 * n * prob / (G * V), (lg, vs)))
    for a, b in zip(*grads):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_argmax_lowest_tie_rule():
    t = torch.tensor([[1.0, 3.0, 3.0, 0.0], [5.0, 5.0, 5.0, 5.0], [0.0, 1.0, 2.0, 2.0]])
    assert K.argmax_lowest(t).tolist() == [1, 0, 2]


def test_ref_sampled_negatives_matches_oracle():
    B, T, N, C, temp = 2, 37, 9, 16, 0.1
    S = B * T
    g = torch.Generator().manual_seed(5)
    cb = torch.randn(7, C, generator=g)
    y = cb[torch.randint(0, 7, (S,), generator=g)]                  # repeated target rows -> masked negatives
    x = torch.randn(S, C, generator=g)
    neg = torch.randint(0, S, (B, T * N), generator=g)
    y[4] = 2.0 * y[10]
    neg[0, 10 * N + 3] = 4                                         # a scaled copy of row 10's positive among its negatives
    x[20] = 0.0                                                    # every logit of row 20 equal (0)
    logits = O.sampled_negatives_logits(x.view(B, T, C), y.view(B, T, C), neg, N, temp)
    want_loss, l2 = O.infonce_loss(logits)
    _, _, log = O.wav2vec_criterion({"x": logits})
    idx = torch.cat([torch.arange(S).view(S, 1), neg.view(B, T, N).reshape(S, N)], dim=1)
    loss, n_correct, got = K.ref_sampled_negatives(x, y, idx, temp)
    want = l2.view(T, B, N + 1).transpose(0, 1).reshape(S, N + 1)   # the criterion's rows are (t, b); the head's (b, t)
    masked = torch.isinf(want)
    assert masked.any() and torch.equal(masked, torch.isinf(got))
    assert not masked[10, 4] and got[10, 4] == got[10, 0]           # the scaled copy is not masked
    torch.testing.assert_close(got[~masked], want[~masked], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(loss, want_loss, rtol=1e-6, atol=1e-6)
    assert n_correct == log["correct"]
    row = got[20]
    assert (row[torch.isfinite(row)] == 0).all()
    # the all-equal row (when none of its negatives is masked it is arg-max = arg-min = 0): never counted as correct
    flat = torch.zeros(3, 5)
    assert K.ref_sampled_negatives(torch.zeros(3, C), torch.randn(8, C, generator=g),
                                   torch.tensor([[0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [2, 3, 4, 5, 6]]), temp)[1] == 0
    assert flat.argmax(-1).tolist() == [0, 0, 0]


def test_chi2_quantile_forms_agree():
    """the Wilson-Hilferty fall-back is within 1 % of scipy's quantile where scipy is present"""
    import math
    from statistics import NormalDist
    for df in (39, 49):
        z = NormalDist().inv_cdf(1.0 - 1e-6)
        wh = df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3
        assert abs(K.chi2_quantile(df) - wh) < 0.01 * wh
