"""Writes tests/golden/transformer_lm_incremental.npz: the reference's TransformerDecoder on the CPU run with `incremental_state`,
one token per call (the path its own FairseqLM switches off, `save_incremental = False`, examples/speech_recognition/
w2l_decoder.py:298), on models A, B and C of tests/transformer_lm_cases.py.  Needs the reference checkout (oracle/ref_shim.py); run
where it is, never on a test machine.  No weights are stored.  Contents, M in A, B, C:
  <M>/rows_<i>   fp32 [T_i, 100]: the full log-prob rows of sentence i of SENTENCES (tests/transformer_lm_cases.py sentences(),
                 the ones of 1, 7 and 33 words), row t the distribution behind [eos, w_1 .. w_t]
  <M>/e_ref      the reference itself in bf16 on the CPU, incrementally: max |bf16 - fp32| over all rows / max |fp32|
  <M>/max        max |fp32| over all rows
  <M>/full_err   max |incremental - full forward| over all rows, fp32 (asserted <= 1e-5)

    python tools/gen_transformer_lm_incremental_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import transformer_lm_cases as C  # noqa: E402
from gen_transformer_lm_golden import build_reference  # noqa: E402

SENTENCES = (1, 2, 3)                  # indices into C.sentences()


def incremental_rows(model, words, dtype):
    """[T, V] fp32: the decoder fed [eos, w_1 .. w_t] with an incremental state, one new token per call"""
    model = model.to(dtype)
    tok = torch.tensor([[C.EOS] + list(words)])
    state, rows = {}, []
    with torch.no_grad():
        for t in range(tok.shape[1]):
            res = model.decoder(tok[:, :t + 1], incremental_state=state)
            assert res[0].shape[1] == 1
            rows.append(model.get_normalized_probs(res, log_probs=True, sample=None)[0, 0].float())
    return torch.stack(rows).numpy()


def full_rows(model, words):
    model = model.to(torch.float32)
    with torch.no_grad():
        res = model(torch.tensor([[C.EOS] + list(words)]))
        return model.get_normalized_probs(res, log_probs=True, sample=None)[0].float().numpy()


def main():
    from oracle import ref_shim
    ref_shim.install()
    out = {}
    for name in C.MODELS:
        model, _ = build_reference(name)
        err = e16 = mx = 0.0
        for i in SENTENCES:                                      # fp32 first: .to(bfloat16) rounds the weights for good
            s = C.sentences()[i]
            rows = incremental_rows(model, s, torch.float32)
            assert rows.shape == (len(s) + 1, C.VOCAB)
            err = max(err, float(np.abs(rows - full_rows(model, s)).max()))
            mx = max(mx, float(np.abs(rows).max()))
            out["%s/rows_%d" % (name, i)] = rows
        for i in SENTENCES:
            rows16 = incremental_rows(model, C.sentences()[i], torch.bfloat16)
            e16 = max(e16, float(np.abs(rows16 - out["%s/rows_%d" % (name, i)]).max()))
        assert err <= 1e-5, (name, err)
        out[name + "/e_ref"] = np.float64(e16 / mx)
        out[name + "/max"] = np.float64(mx)
        out[name + "/full_err"] = np.float64(err)
        print("model %s: incremental against the full forward %.3e, max |log-prob| %.3f, bf16 reference on the CPU e_ref %.3e"
              % (name, err, mx, e16 / mx))
    path = os.path.join(ROOT, "tests", "golden", "transformer_lm_incremental.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
