"""csrc/resample.hip on the device against resample_reference run on the table the kernel reads (fp32-rounded), in float64.

The bound is derived, not tuned: an output is a chain of T = 2 * width + 1 fmaf's in fp32, so per sample
    |err| <= E = (T + 1) * 2^-24 * sum_k |h_i[k]| * |x_k|
(T roundings of the running sum, each at most 2^-24 of a partial sum that the sum of magnitudes bounds; the +1 leaves room for
the second-order terms).  bf16 output adds 2^-9 * |y| to that bound.  The tests assert against TWICE the bound, computed per
sample from the table and the input: 2 E for fp32 output, 2 E + 2^-8 * |y| for bf16.  The bf16 term doubled is exactly the
format's unit roundoff (8 significant bits: a correctly rounded value is off by up to 2^-8 of itself; no kernel can stay
within 2^-9 * |y|, e.g. 0.2645 lies 8.3e-4 from its nearest bf16 neighbour 0.263671875, and 2^-9 * 0.2645 = 5.2e-4), and the
bf16 output is also required to EQUAL the fp32 output rounded once to nearest-even, which is stricter than either figure.
int16 input is compared against the oracle fed pcm / 32768, which is exact in fp32."""
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RATIOS = [(8000, 16000), (16000, 8000), (48000, 16000), (44100, 16000), (11025, 16000)]
LENGTHS = [1, 5, 1000, 70001]   # 5 < width for every ratio; 70001 crosses several workgroup tiles and n * L / o is no integer
B = 3

_TABLE32, _CASES = {}, {}


def table32(orig, new):
    """the dense [n, 2 * width + o] filter rebuilt from what the kernel is handed: compact taps rounded to fp32"""
    from unispeech_amd.resample import compact_table
    if (orig, new) not in _TABLE32:
        taps, first, width, o, n = compact_table(orig, new)
        dense = np.zeros((n, 2 * width + o))
        for i in range(n):
            dense[i, first[i]:first[i] + taps.shape[1]] = taps[i].astype(np.float32).astype(np.float64)
        _TABLE32[(orig, new)] = (dense, width, o, n)
    return _TABLE32[(orig, new)]


def oracle(x, orig, new):
    """-> (y float64, E float64: the per-sample bound of the module docstring) for x [.., L]"""
    from unispeech_amd.resample import resample_reference
    dense, width, o, n = table32(orig, new)
    x = torch.as_tensor(x).double()
    y = resample_reference(x, orig, new, table=dense)
    mag = resample_reference(x.abs(), orig, new, table=np.abs(dense))
    return y, (2 * width + 2) * 2.0 ** -24 * mag


def case(orig, new, L):
    """one input per (ratio, L), its int16 image and both oracles, computed once and shared (never modified)"""
    key = (orig, new, L)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * L + orig % 997)
        x = torch.randn(B, L, generator=g).clamp_(-1, 1)
        pcm = torch.round(x * 32767).to(torch.int16)
        _CASES[key] = (x, pcm, oracle(x, orig, new), oracle(pcm.double() / 32768.0, orig, new))
    return _CASES[key]


def check(got, want, bound, what, lowp=False):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    tol = 2.0 * (bound + (2.0 ** -9 * want.abs() if lowp else 0.0))
    err = (got - want).abs()
    print("%s: max error %.3e, max bound %.3e, worst error / bound %.3f" % (
        what, err.max().item(), tol.max().item(), (err / tol.clamp_min(1e-300)).max().item()))
    assert bool((err <= tol).all()), what


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("rates", RATIOS)
def test_matches_the_float64_oracle(rates, L):
    from unispeech_amd.resample import Resample, output_length, resample
    orig, new = rates
    x, pcm, (y, bound), (yi, boundi) = case(orig, new, L)
    _, _, o, n = table32(orig, new)
    assert y.shape == (B, math.ceil(n * L / o)) and y.shape[1] == output_length(L, o, n)
    got = resample(x.cuda(), orig, new)
    assert got.dtype == torch.float32
    check(got, y, bound, "%d->%d L=%d fp32" % (orig, new, L))
    check(resample(pcm.cuda(), orig, new), yi, boundi, "%d->%d L=%d int16 in" % (orig, new, L))
    low = resample(x.cuda(), orig, new, out_dtype=torch.bfloat16)
    assert low.dtype == torch.bfloat16
    check(low, y, bound, "%d->%d L=%d bf16 out" % (orig, new, L), lowp=True)
    assert torch.equal(low, got.bfloat16())                          # the same sums, rounded once
    mod = Resample(orig, new)(x.cuda().view(B, 1, L))
    assert mod.shape == (B, 1, y.shape[1]) and torch.equal(mod.view(B, -1), got)
    assert torch.equal(resample(x[0].cuda(), orig, new), got[0])     # 1-D in, 1-D out


@pytest.mark.parametrize("rates,L", [((8000, 16000), 70001), ((44100, 16000), 70001), ((16000, 8000), 1000),
                                     ((48000, 16000), 1000), ((11025, 16000), 1000)])
def test_lengths_equal_each_row_alone_and_the_rest_is_zero(rates, L):
    from unispeech_amd.resample import output_length, resample
    orig, new = rates
    x, _, _, _ = case(orig, new, L)
    _, _, o, n = table32(orig, new)
    lens = [L, L // 2, 1]
    xd = x.cuda()
    out = torch.full((B, output_length(L, o, n)), 7.0, device="cuda")
    got = resample(xd, orig, new, lengths=lens, out=out)
    assert got is out
    for r, ln in enumerate(lens):
        k = output_length(ln, o, n)
        alone = resample(xd[r:r + 1, :ln].contiguous(), orig, new)
        assert alone.shape == (1, k)
        assert torch.equal(got[r, :k], alone[0]), (r, ln)
        assert bool((got[r, k:] == 0).all()), (r, ln)
        y, bound = oracle(x[r, :ln], orig, new)
        check(got[r, :k], y, bound, "%d->%d row %d length %d" % (orig, new, r, ln))
    glen = resample(xd, orig, new, lengths=torch.tensor(lens, device="cuda"), out_dtype=torch.bfloat16)
    assert torch.equal(glen, got.bfloat16())


@pytest.mark.parametrize("rates", RATIOS)
def test_a_row_does_not_depend_on_its_batch_and_two_runs_agree(rates):
    from unispeech_amd.resample import resample
    orig, new = rates
    x = case(orig, new, 70001)[0].cuda()
    a = resample(x, orig, new).clone()
    b = resample(x, orig, new)
    assert torch.equal(a, b)
    assert torch.equal(resample(x[1:2].contiguous(), orig, new)[0], a[1])
    assert torch.equal(resample(torch.cat([x[2:3], x[1:2], x[0:1], x[1:2], x[1:2]]), orig, new)[3], a[1])


@pytest.mark.parametrize("rates", [(8000, 16000), (44100, 16000)])
def test_strided_rows_and_untouched_surroundings(rates):
    from unispeech_amd.resample import resample
    orig, new = rates
    L = 1000
    x, pcm, _, _ = case(orig, new, L)
    for src in (x, pcm):
        want = resample(src.cuda(), orig, new)
        wide_in = torch.full((B, L + 37), 3, dtype=src.dtype).cuda()
        wide_in[:, 5:5 + L] = src.cuda()
        view = wide_in[:, 5:5 + L]
        assert not view.is_contiguous()
        assert torch.equal(resample(view, orig, new), want)
        for dtype in (torch.float32, torch.bfloat16):
            wide = torch.full((B + 1, want.shape[1] + 29), -5.0, dtype=dtype, device="cuda")
            out = wide[:B, 3:3 + want.shape[1]]
            resample(view, orig, new, out=out)
            assert torch.equal(out, want.to(dtype))
            wide[:B, 3:3 + want.shape[1]] = -5.0
            assert bool((wide == -5.0).all())


def test_predict_resamples_chunk_by_chunk_on_the_device():
    """2.2 chunks at chunk_size 50, sr 8000, frame_shift 320: the batch that reaches the head is the per-chunk oracle, and it is
    NOT the whole recording resampled and then cut -- the two differ where the filter reaches across a seam"""
    from unispeech_amd.diarization import predict
    from unispeech_amd.resample import resample_reference
    seen = []

    def batch_estimate(chunks):
        seen.append(chunks)
        return torch.zeros(len(chunks), 50, 2), torch.ones(len(chunks), 2, 4)

    stub = types.SimpleNamespace(sr=8000, frame_shift=320, subsampling=1, batch_estimate=batch_estimate)
    size = 50 * 320
    n8 = int(2.2 * size)
    g = torch.Generator().manual_seed(8)
    wav8 = torch.randn(n8, generator=g).clamp_(-1, 1)
    acti, svec, lens = predict(stub, wav8.cuda(), 50, input_rate=8000)
    assert lens == [50, 50, 10] and [a.shape for a in acti] == [(50, 2), (50, 2), (10, 2)]
    assert len(seen) == 1 and seen[0].is_cuda and tuple(seen[0].shape) == (3, 2 * size)
    spans = [(0, size), (size, 2 * size), (n8 - size, n8)]
    dense = table32(8000, 16000)[0]
    whole = resample_reference(wav8, 8000, 16000, table=dense)
    for c, (s, e) in enumerate(spans):
        y, bound = oracle(wav8[s:e], 8000, 16000)
        check(seen[0][c], y, bound, "chunk %d" % c)
        cut = whole[2 * s:2 * e]
        d = (y - cut).abs()
        assert d[50:-50].max().item() < 1e-12                        # away from the seams the two are one computation
        if s > 0:
            assert d[:14].max().item() > 100 * bound[:14].max().item(), c   # the chunk's own zero padding instead of its neighbour
        if e < n8:
            assert d[-14:].max().item() > 100 * bound[-14:].max().item(), c
    got = seen[0].double().cpu()
    assert (got[1] - whole[2 * size:4 * size]).abs()[:14].max().item() > 1e-3


def test_speaker_cli_embeds_an_8_khz_file(tmp_path, capsys):
    from test_speaker import write_wav, z
    from test_speaker_gpu import build_e2e
    from unispeech_amd import speaker
    from unispeech_amd.resample import resample
    g = z()
    m, cfgd = build_e2e(g, "e2e_tiny")
    up = m.feature_extract.model
    torch.save({"cfg": cfgd, "model": {k: v.cpu() for k, v in up.state_dict().items()}}, tmp_path / "up.pt")
    torch.save({"model": {k: v.cpu() for k, v in m.state_dict().items()}}, tmp_path / "head.pt")
    pcm = g["e2e_tiny/wav_i16"][0][:16000]                           # 2 s when read as 8 kHz audio
    write_wav(tmp_path / "a8.wav", pcm, sr=8000)
    speaker.main(["embed", str(tmp_path / "up.pt"), str(tmp_path / "head.pt"), str(tmp_path / "a8.wav")])
    words = capsys.readouterr().out.strip().split()
    emb = np.array([float(w) for w in words[1:]])
    assert words[0] == str(tmp_path / "a8.wav") and emb.shape == (256,) and np.isfinite(emb).all() and np.abs(emb).max() > 0
    wav16 = resample(torch.from_numpy(pcm.astype(np.float32) / 32768.0).cuda(), 8000, 16000)
    assert wav16.shape == (32000,)
    with torch.no_grad():
        want = m([wav16]).float().cpu().numpy()[0]
    assert np.abs(emb - want).max() <= 1e-6 + 1e-5 * np.abs(want).max()     # the printed six decimals of the same computation
