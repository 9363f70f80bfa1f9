"""csrc/fbank.hip on the device against fbank_reference (tests/fbank_cases.py holds the inputs and both oracles), and the
fbank speaker model against the reference's outputs in tests/golden/speaker_fbank.npz (tools/gen_speaker_fbank_golden.py).

Tolerance of the front end: measured on the reference side, never on the device's.  For a case -- the rows of one length --
E32[m] is the largest |fbank_reference(float32) - fbank_reference(float64)| of mel column m over the frames of the case's rows:
what the reference's own precision (fp32 window and filters, fp32 pocketfft, fp32 sums and log) costs on that input.  The
device must lie within 4 x E32[m] of the float64 value in every frame and column: the convention and the factor of
tests/test_mfcc_gpu.py, for the same transform.  The worst ratio per case is printed (-s).
Model: the fp32 head tolerances of tests/test_speaker_gpu.py (5e-4 of the tensor's max magnitude, 1e-3 on the cosine: the same
head and kernels), bf16 within twice the reference's own bf16 error."""
import numpy as np
import pytest
import torch

import fbank_cases as FC
from conftest import load_golden
from test_speaker import cos_matrix, fill_state_dict, ramp, write_wav

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def leave_no_device_memory_behind():
    """the front end's device tables and the head's scratch buffer are cached for the life of the process; drop them when this
    module is done, so that later modules meet the caching allocator as they did before this one existed"""
    yield
    import gc
    from unispeech_amd import fbank, ops
    fbank._TABLES.clear()
    for key in [k for k in ops._WS if k[1] == "spk"]:
        del ops._WS[key]
    gc.collect()
    torch.cuda.empty_cache()


def _dev(pcm, dtype):
    t = torch.from_numpy(np.array(pcm))
    return (t if dtype == torch.int16 else t.to(torch.float32) / 32768.0).cuda()


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------------------- front end
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["fp32", "int16"])
@pytest.mark.parametrize("L", FC.LENGTHS)
def test_parity(L, dtype):
    from unispeech_amd.fbank import fbank, frames
    rows = FC.case_rows(L)
    E = FC.e32(rows)
    T = frames(L)
    assert T == {257: 2, 1600: 11, 16037: 101}[L] and (E > 0).all()
    got = fbank(torch.stack([_dev(p, dtype) for p in rows]))
    assert got.shape == (len(rows), T, 40) and got.dtype == torch.float32
    worst = 0.0
    for r, p in enumerate(rows):
        err = np.abs(f64(got[r]) - FC.refs(p)[0])                            # every frame, every column
        worst = max(worst, float((err / E[None, :]).max()))
    print("fbank parity L=%d %s: worst |dev - f64| / E32 = %.3f (E32 %.3e .. %.3e)" % (L, dtype, worst, E.min(), E.max()))
    assert worst <= 4.0
    # the 1-D form and a strided view of a wider buffer read the same
    assert torch.equal(fbank(_dev(rows[0], dtype)), got[0])
    wide = torch.zeros(len(rows), L + 7, dtype=got.dtype if dtype != torch.int16 else torch.int16, device="cuda")
    wide[:, :L] = torch.stack([_dev(p, dtype) for p in rows])
    assert torch.equal(fbank(wide[:, :L]), got)


def test_int16_equals_fp32_of_the_scaled_samples():
    from unispeech_amd.fbank import fbank
    p = FC.case_rows(1600)[0]
    assert torch.equal(fbank(_dev(p, torch.int16)), fbank(_dev(p, torch.float32)))


def test_silence():
    """an all-zero row has an all-zero spectrum: logf(1e-6f) in every column (the device's logf within one ulp of the correctly
    rounded value), and the instance norm of that constant column is exactly zero"""
    from unispeech_amd.fbank import fbank
    from unispeech_amd.speaker import ECAPA_TDNN_SMALL
    x = torch.zeros(2, 1600 + 37, device="cuda")
    y = fbank(x)
    assert y.shape == (2, 11, 40) and (y == y[0, 0, 0]).all()
    want = np.float32(np.log(np.float64(np.float32(1e-6))))
    assert abs(float(y[0, 0, 0]) - float(want)) <= abs(float(np.spacing(want))), (float(y[0, 0, 0]), float(want))
    # through the model's norm: silence beside a live row, one call
    m = ECAPA_TDNN_SMALL(feat_dim=40, feat_type="fbank")
    m.load_state_dict(fill_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("feature_extract.")}, 9),
                      strict=False)
    m = m.cuda().eval()
    live = _dev(FC.case_rows(1600)[0], torch.float32)
    inter = {}
    with torch.no_grad():
        emb = m([torch.zeros(1600, device="cuda"), live, torch.zeros(900, device="cuda")], intermediates=inter)
    n = inter["normed"]
    assert n.shape == (3, 11, 40) and (n[0] == 0).all() and (n[2] == 0).all() and float(n[1].abs().max()) > 0.5
    assert torch.isfinite(emb).all()


def test_batching():
    """B = 3 rows of 257, 1600 and 16037 samples in one call: each row's bits are those of the row alone, frames beyond a row's
    count are zero, what lies beyond a row's length is never read into the features, two runs agree bit for bit"""
    from unispeech_amd.fbank import fbank, frames
    rows = [FC.case_rows(L)[0] for L in FC.LENGTHS]
    lens = [len(p) for p in rows]
    pcm = np.full((3, max(lens)), 12345, np.int16)
    for r, p in enumerate(rows):
        pcm[r, :lens[r]] = p
    x32 = torch.from_numpy(pcm).cuda().to(torch.float32) / 32768.0
    got = fbank(x32, lengths=lens)
    assert got.shape == (3, 101, 40)
    for r, p in enumerate(rows):
        n = frames(lens[r])
        alone = fbank(_dev(p, torch.float32))
        assert alone.shape == (n, 40) and torch.equal(alone, got[r, :n])
        assert (got[r, n:] == 0).all()
    assert torch.equal(fbank(x32, lengths=torch.tensor(lens)), got)
    assert torch.equal(fbank([_dev(p, torch.float32) for p in rows]), got)      # the list form pads with zeros: same bits
    assert torch.equal(fbank(x32[[2, 0, 1]], lengths=[lens[2], lens[0], lens[1]]), got[[2, 0, 1]])
    short = fbank(x32, lengths=[256, 0, 16037])                              # rows too short to reflect: no frames
    assert (short[:2] == 0).all() and torch.equal(short[2], got[2])


# ----------------------------------------------------------------------------------------------------------------- model
def build(g, dtype=torch.float32):
    from unispeech_amd.speaker import ECAPA_TDNN_SMALL
    m = ECAPA_TDNN_SMALL(feat_dim=40, feat_type="fbank")
    head = fill_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("feature_extract.")}, int(g["seed_w"]))
    r = m.load_state_dict(head, strict=False)
    assert r.unexpected_keys == []
    return m.to(dtype).cuda().eval()


def waves(g):
    return [torch.from_numpy(w).cuda() for w in FC.golden_waves(int(g["seed_x"]))]


def rel(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(f64(got) - want).max() / np.abs(want).max()


def test_model_fp32_vs_reference():
    """four unequal waveforms in ONE call against the reference run on each file alone"""
    g = load_golden("speaker_fbank.npz")
    m, wavs = build(g), waves(g)
    inter = {}
    with torch.no_grad():
        emb = m(wavs, intermediates=inter)
        one = torch.cat([m([w]) for w in wavs])
    frames = [1 + len(w) // 160 for w in wavs]
    n = f64(inter["normed"])
    chk = np.stack([(n[b, :T] * ramp(T)[:, None]).sum(0) for b, T in enumerate(frames)])
    assert all((n[b, T:] == 0).all() for b, T in enumerate(frames))
    figs = dict(normed_chk=rel(torch.from_numpy(chk), g["normed_chk"]), emb=rel(emb, g["emb"]), one_per_file=rel(one, g["emb"]),
                batch_vs_files=rel(emb, f64(one)))
    cerr = np.abs(cos_matrix(f64(emb)) - g["cos"]).max()
    print("fbank model fp32:", figs, "cos", cerr)
    assert emb.shape == (4, 256) and all(v <= 5e-4 for v in figs.values()), figs
    assert cerr <= 1e-3, cerr


def test_model_bf16_within_twice_the_reference_bf16_error():
    g = load_golden("speaker_fbank.npz")
    m, wavs = build(g, torch.bfloat16), waves(g)
    with torch.no_grad():
        emb = m(wavs)
        again = m(wavs)
    e_ref, c_ref = float(g["e_ref"]), float(g["cos_err_bf16"])
    e = rel(emb, g["emb"])
    cerr = np.abs(cos_matrix(f64(emb)) - g["cos"]).max()
    print("fbank model bf16: error %.3e (e_ref %.3e), cosine error %.3e (reference bf16 %.3e)" % (e, e_ref, cerr, c_ref))
    assert emb.dtype == torch.bfloat16 and e <= 2 * e_ref, (e, e_ref)
    assert cerr <= 2 * c_ref, (cerr, c_ref)
    assert torch.equal(emb, again)


def test_cli_verify_prints_the_reference_sentence(tmp_path, capsys):
    from unispeech_amd import speaker
    g = load_golden("speaker_fbank.npz")
    m = build(g)
    torch.save({"model": {k: v.cpu() for k, v in m.state_dict().items()}}, tmp_path / "head.pt")
    w = FC.golden_waves(int(g["seed_x"]))
    for i in (0, 3):
        write_wav(tmp_path / ("%d.wav" % i), np.round(w[i] * 32768.0).astype(np.int16))
    speaker.main(["verify", "--fbank", str(tmp_path / "head.pt"), str(tmp_path / "0.wav"), str(tmp_path / "3.wav")])
    out = capsys.readouterr().out.strip()
    assert out.startswith("The similarity score between two audios is ") and out.endswith(" (-1.0, 1.0).")
    assert abs(float(out.split()[-3]) - float(g["cos"][0, 3])) <= 1e-3, (out, float(g["cos"][0, 3]))
