"""Utterance / noise mixing + collation against tests/golden/mixing.npz, which oracle/gen_golden.py
produced by calling the reference's `UtteranceMixingDataset.collater` (src/fairseq/data/audio/utterance_mixing_dataset.py:
323-438) under fixed numpy seeds.

CPU: the host side of the product (unispeech_amd.data.UtteranceMixingCollater: crops, mixing plan, label collation) consumes
the numpy stream exactly as the reference (same next draw), padding mask and labels are bit-exact, and the oracle's
restatement of the mixing arithmetic applied to that plan reproduces the reference's waveform batch to 1e-6.
GPU: the device kernel (wavlm_mix_utterances) applied to the same plan matches the golden to 1e-6 of the batch scale
(float32 power reductions are summed in a different order than numpy's pairwise sum; everything else is the same
arithmetic), and its bf16 output equals the bf16 rounding of its fp32 output.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden


def _inputs(z):
    n = len(z["in/lens"])
    audios = [torch.from_numpy(z["in/audio%d" % i]) for i in range(n)]
    labels = [torch.from_numpy(z["in/label%d" % i]) for i in range(n)]
    return [{"id": i, "source": a.clone(), "label_list": [l.clone()], "boundary": []} for i, (a, l) in enumerate(zip(audios, labels))]


def _collaters(z, device=None, out_dtype=torch.float32):
    from unispeech_amd.data import UtteranceMixingCollater
    offs = z["in/noise_offs"]
    cat = z["in/noise_i16"]
    nlist = [{"loc": "bank\tk%d\t%d\t%d" % (i, offs[i], offs[i + 1])} for i in range(3)]

    def loader(entry):  # what the reference does with its h5 container (utterance_mixing_dataset.py:386-390)
        _p, _k, s, e = entry["loc"].split("\t")
        return cat[int(s):int(e)].astype(np.float32) / np.iinfo(np.int16).max

    utt = UtteranceMixingCollater(label_rates=[50], pad_list=[1], max_sample_size=4600, pad_audio=False, normalize=True,
                                  random_crop=True, mixing_prob=0.7, mixing_num=2, device=device, out_dtype=out_dtype)
    noise = UtteranceMixingCollater(label_rates=[50], pad_list=[1], max_sample_size=5600, pad_audio=True, normalize=False,
                                    random_crop=True, mixing_prob=0.9, mixing_num=1, mixing_noise=True,
                                    mixing_noise_prob=0.6, mixing_noise_num=2, noise_list=nlist, noise_loader=loader,
                                    device=device, out_dtype=out_dtype)
    return {"utt": (utt, 4711), "noise": (noise, 1213)}


@pytest.mark.parametrize("tag", ["utt", "noise"])
def test_host_plan_labels_and_oracle_mixing_vs_reference_collater(tag):
    from oracle import wavlm_oracle as O
    z = load_golden("mixing.npz")
    col, seed = _collaters(z)[tag]
    np.random.seed(seed)
    b = col.collater(_inputs(z))
    assert np.random.random() == float(z[tag + "/next"]), "numpy stream consumption differs from the reference collater"
    assert torch.equal(b["net_input"]["padding_mask"], torch.from_numpy(z[tag + "/padding_mask"]))
    assert torch.equal(b["target_list"][0], torch.from_numpy(z[tag + "/target"]))
    assert torch.equal(b["target_lengths_list"][0], torch.from_numpy(z[tag + "/target_lengths"]))
    assert b["ntokens_list"][0] == int(z[tag + "/ntokens"])
    ops, begin, noise = b["mixing_plan"]
    assert ops.shape[0] >= 3
    mixed = O.mix_collated_audios(b["net_input"]["source"], ops, begin, noise, normalize=col.normalize)
    ref = torch.from_numpy(z[tag + "/source"])
    assert mixed.shape == ref.shape
    assert (mixed - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
    assert (b["net_input"]["source"] - ref).abs().max().item() > 1e-3, "the fixture must actually mix something"


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["utt", "noise"])
def test_device_mixing_kernel_vs_reference_collater(tag):
    z = load_golden("mixing.npz")
    col, seed = _collaters(z, device="cuda")[tag]
    np.random.seed(seed)
    b = col.collater(_inputs(z))
    src = b["net_input"]["source"]
    assert src.is_cuda and src.dtype == torch.float32
    ref = torch.from_numpy(z[tag + "/source"])
    err = (src.cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err <= 1e-6, err
    assert torch.equal(b["net_input"]["padding_mask"].cpu(), torch.from_numpy(z[tag + "/padding_mask"]))
    assert torch.equal(b["target_list"][0], torch.from_numpy(z[tag + "/target"]))
    col16, _ = _collaters(z, device="cuda", out_dtype=torch.bfloat16)[tag]
    np.random.seed(seed)
    b16 = col16.collater(_inputs(z))
    assert b16["net_input"]["source"].dtype == torch.bfloat16
    assert torch.equal(b16["net_input"]["source"], src.to(torch.bfloat16))


@pytest.mark.gpu
def test_device_mixing_at_batch_scale_dependency_chain():
    """32 x 15 s (the bench batch): every row mixed twice, partners chosen so that long chains of "finished lower row"
    dependencies and self-mixes occur; compared with the oracle's sequential restatement on the same plan."""
    from oracle import wavlm_oracle as O
    from unispeech_amd import ops as K
    B, T = 32, 240000
    g = torch.Generator().manual_seed(5)
    src = torch.randn(B, T, generator=g) * 0.1
    rs = np.random.RandomState(9)
    plan, begin = [], [0]
    for i in range(B):
        for c in (max(i - 1, 0), int(rs.randint(0, B))):       # i-1: a chain through all rows; plus a random partner
            c_len = int(rs.randint(0, T // 2 + 1))
            c_end, s_end = int(rs.randint(c_len, T + 1)), int(rs.randint(c_len, T + 1))
            gain = np.float32(10 ** (rs.uniform(-5, 5) / 10)).view(np.int32)
            plan.append((i, 0, c, c_end - c_len, s_end - c_len, c_len, T, int(gain)))
        begin.append(len(plan))
    ops = np.asarray(plan, dtype=np.int32)
    begin = np.asarray(begin, dtype=np.int32)
    want = O.mix_collated_audios(src, ops, begin, None, normalize=True)
    got = K.mix_utterances(src.cuda(), torch.from_numpy(ops.reshape(-1)).cuda(), ops.shape[0], torch.from_numpy(begin).cuda(),
                           None, True)
    err = (got.cpu() - want).abs().max().item() / want.abs().max().item()
    assert err <= 2e-6, err


@pytest.mark.gpu
def test_collater_feeds_the_pretraining_step():
    """the batch dict of UtteranceMixingCollater goes into the criterion unchanged (the reference's
    `utterance_mixing_pretraining` task -> `wavlm` criterion hand-over): device waveform already mixed and bf16-cast,
    host copy of the padding mask, boundary list, label tensors; one forward + backward of the tiny model."""
    from conftest import TINY, golden_state_dict
    from unispeech_amd.pretrain import WavLMCriterion, WavLMPretrainConfig, WavLMPretrainModel
    z = load_golden("mixing.npz")
    zt = load_golden("tiny_pretrain.npz")
    cfg = WavLMPretrainConfig(**{k: v for k, v in TINY.items() if k in WavLMPretrainConfig.__dataclass_fields__})
    model = WavLMPretrainModel(cfg, None, [range(23)])
    model.load_state_dict(golden_state_dict(zt))
    model = model.cuda().to(torch.bfloat16).train()
    col, seed = _collaters(z, device="cuda", out_dtype=torch.bfloat16)["noise"]
    np.random.seed(seed)
    batch = col.collater(_inputs(z))
    assert batch["net_input"]["source"].dtype == torch.bfloat16 and batch["net_input"]["padding_mask"].any()
    batch["target_list"] = [t.cuda() for t in batch["target_list"]]
    batch.pop("mixing_plan")
    crit = WavLMCriterion(None, 1.0, 0.0, loss_weights=[10.0])
    loss, ss, log = crit(model, batch)
    loss.backward()
    assert torch.isfinite(loss) and ss > 0 and log["nsentences"] == 6
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


def test_silent_crop_of_a_non_silent_utterance_follows_the_reference_stream():
    """The reference measures the partner's power on the COLLATED row (after the crop, utterance_mixing_dataset.py:420-426):
    an utterance whose kept crop is digital silence gets no SNR draw although the utterance itself is not silent.  The
    reference collater's batches and next numpy draws (tests/golden/mixing_silent_crop.npz, oracle/gen_golden.py) against the
    product's host plan: same next numpy draw, same mixed batch, and the last stored seed's plan takes the silent-crop row as a
    partner."""
    from oracle import wavlm_oracle as O
    from unispeech_amd.data import UtteranceMixingCollater
    z = load_golden("mixing_silent_crop.npz")
    n = len(z["in/lens"])
    audios = [torch.from_numpy(z["in/audio%d" % i]) for i in range(n)]
    labels = [torch.from_numpy(z["in/label%d" % i]) for i in range(n)]
    assert not (audios[1][:4000] != 0).any() and (audios[1][4000:] != 0).any()   # crop [0:4000] (random_crop off) is silent

    def samples():
        return [{"id": i, "source": a.clone(), "label_list": [l.clone()], "boundary": []}
                for i, (a, l) in enumerate(zip(audios, labels))]

    hit = None
    for seed in range(int(z["seeds"])):
        col = UtteranceMixingCollater(label_rates=[50], pad_list=[1], pad_audio=False, normalize=False, random_crop=False,
                                      mixing_prob=1.0, mixing_num=3)
        np.random.seed(seed)
        b = col.collater(samples())
        assert np.random.random() == float(z["seed%d/next" % seed]), "numpy stream diverged from the reference (seed %d)" % seed
        ops, begin, noise = b["mixing_plan"]
        mixed = O.mix_collated_audios(b["net_input"]["source"], ops, begin, noise, normalize=False)
        ref = torch.from_numpy(z["seed%d/source" % seed])
        assert (mixed - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
        if any(int(o[1]) == 0 and int(o[2]) == 1 for o in ops):
            hit = seed
            break
    assert hit == int(z["seeds"]) - 1, "no plan used the silent-crop row as a partner"


def test_staging_buffers_rotate():
    """consecutive collations never hand out the staging buffer of the previous batch (its asynchronous H2D copy may still
    be pending); a buffer comes back only after `len(_stages)` further batches, guarded by the copy's event"""
    from unispeech_amd.data import UtteranceMixingCollater
    col = UtteranceMixingCollater(mixing_prob=0.0)
    ptrs = [col._staging(2, 100).data_ptr() for _ in range(6)]
    n = len(col._stages)
    assert n >= 2 and len(set(ptrs[:n])) == n and ptrs[:n] == ptrs[n:2 * n]
