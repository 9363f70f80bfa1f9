"""Branches of the HIP path that the golden / oracle parity tests do not reach: deferred (device-side) logging,
`padding_mask_cpu`, encoder_layerdrop > 0, empty frame selections, out-of-range labels, optimizer checkpoints, and the
RCCL transport of the gradient reducer (world 2, only where two GPUs are visible)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

from conftest import TINY, golden_state_dict, load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(golden="tiny_pretrain.npz", **over):
    from unispeech_amd.pretrain import WavLMPretrainConfig, WavLMPretrainModel
    z = load_golden(golden)
    d = dict(TINY)
    d.update(over)
    cfg = WavLMPretrainConfig(**{k: v for k, v in d.items() if k in WavLMPretrainConfig.__dataclass_fields__})
    m = WavLMPretrainModel(cfg, None, [range(23)])
    m.load_state_dict(golden_state_dict(z))
    return m.cuda().train(), z


def _sample(z, cpu_mask=False):
    pm = torch.from_numpy(z["in/padding_mask"])
    ni = {"source": torch.from_numpy(z["in/source"]).cuda(), "padding_mask": pm.cuda()}
    if cpu_mask:
        ni["padding_mask_cpu"] = pm
    return {"id": torch.arange(2), "net_input": ni, "target_list": [torch.from_numpy(z["in/target"]).cuda()]}


def test_deferred_logging_and_host_padding_mask_match_eager_path():
    """defer_logging=True keeps every logging value a device tensor (no .item() per micro-batch) and `padding_mask_cpu`
    removes the forward's only device->host copy: both must give exactly the numbers of the eager path, which the
    golden test pins against the reference."""
    from unispeech_amd.pretrain import WavLMCriterion
    model, z = _tiny()
    eager = WavLMCriterion(None, 1.0, 0.0, loss_weights=[10.0])
    lazy = WavLMCriterion(None, 1.0, 0.0, loss_weights=[10.0], defer_logging=True)
    np.random.seed(123)
    l0, s0, g0 = eager(model, _sample(z))
    np.random.seed(123)
    l1, s1, g1 = lazy(model, _sample(z, cpu_mask=True))
    assert s0 == s1 and l0.item() == l1.item()
    assert g0.keys() == g1.keys()
    for k in g0:
        v = g1[k]
        if k in ("loss", "loss_m_0", "loss_u_0", "loss_features_pen", "correct_m_0", "correct_u_0"):
            assert torch.is_tensor(v) and v.is_cuda, k   # really deferred
        assert float(v) == float(g0[k]), k
    assert abs(float(g0["loss"]) - float(z["out/loss"])) < 1e-4 * abs(float(z["out/loss"]))
    a = WavLMCriterion.reduce_metrics([g0])
    b = WavLMCriterion.reduce_metrics([g1])
    assert a == b


def test_encoder_layerdrop_skips_layers_and_keeps_numpy_stream():
    """encoder_layerdrop > 0 (hubert pretrain.sh uses 0.05): a dropped layer is the identity, its parameters get no
    gradient, and the host numpy stream advances exactly one draw per layer as in the reference (wavlm.py:726-731)."""
    from unispeech_amd.pretrain import WavLMCriterion
    model, z = _tiny(encoder_layerdrop=0.5)
    crit = WavLMCriterion(None, 1.0, 0.0, loss_weights=[10.0])
    seen = set()
    for seed in range(40, 60):
        np.random.seed(seed)
        from unispeech_amd.masking import compute_mask_indices
        compute_mask_indices((2, 49), torch.zeros(2, 49, dtype=torch.bool), 0.65, 4, "static", 0, min_masks=2)
        draws = [np.random.random() for _ in range(2)]
        nxt = np.random.random()
        dropped = tuple(d <= 0.5 for d in draws)
        if dropped in seen:
            continue
        seen.add(dropped)
        model.zero_grad()
        np.random.seed(seed)
        loss, _, _ = crit(model, _sample(z))
        assert np.random.random() == nxt, "numpy stream consumption differs from one draw per layer"
        loss.backward()
        assert torch.isfinite(loss)
        for li, dr in enumerate(dropped):
            g = model.encoder.layers[li].fc1.weight.grad
            if dr:
                assert g is None or float(g.abs().max()) == 0.0, (seed, li)
            else:
                assert g is not None and float(g.abs().max()) > 0.0, (seed, li)
    assert len(seen) >= 3


def test_empty_frame_selection_and_bad_labels():
    """mask=False: the masked head sees an EMPTY frame set (S = 0) -- the reference yields empty logits and a zero loss;
    the GEMM / gather entry points reject M = 0, so the host layer must short-circuit.  A label outside the dictionary
    makes the loss NaN (device labels: no host read-back) or raises IndexError (host labels), never an OOB read."""
    from unispeech_amd.pretrain import WavLMCriterion
    model, z = _tiny()
    s = _sample(z)
    net = model(target_list=s["target_list"], mask=False, **s["net_input"])
    h = net["masked"][0]
    assert h["count"] == 0 and float(h["loss"]) == 0.0
    assert model.get_logits(net, True)[0].shape[0] == 0
    (h["loss"].sum() + net["nomask"][0]["loss"].sum() * 0).backward()   # backward through the empty head must work too
    crit = WavLMCriterion(None, 1.0, 0.0, loss_weights=[10.0])
    bad = _sample(z)
    bad["target_list"][0] = bad["target_list"][0].clone()
    bad["target_list"][0][0, 3:20] = 23                                    # == len(dictionary): out of range
    np.random.seed(123)
    loss, _, _ = crit(model, bad)
    assert torch.isnan(loss)
    bad["target_list"][0] = bad["target_list"][0].cpu()
    with pytest.raises(IndexError):
        crit(model, bad)


def test_fused_adam_checkpoint_roundtrip_and_rehoming():
    """state_dict() carries the arena layout; loading into the same layout restores the run bit-exactly, loading into an
    arena laid out differently (no q|k|v packing) re-homes every parameter by name, and a layout mismatch without names
    raises instead of silently misaligning the moments.  fairseq-shaped per-parameter state round-trips as well."""
    from unispeech_amd.optim import FusedAdam
    from unispeech_amd.pretrain import WavLMCriterion
    crit = WavLMCriterion(None, 1.0, 0.0, loss_weights=[10.0])

    def run(model, opt, steps, seed0):
        for i in range(steps):
            opt.zero_grad()
            np.random.seed(seed0 + i)
            loss, ss, _ = crit(model, _sample(z))
            loss.backward()
            opt.step(grad_mult=1.0 / ss)

    model, z = _tiny()
    names = [n for n, _ in model.named_parameters()]
    opt = FusedAdam(model.parameters(), lr=1e-3, model=model)
    run(model, opt, 2, 10)
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict(names=names).items()}
    msd = {k: v.clone() for k, v in model.state_dict().items()}
    run(model, opt, 2, 20)
    # same layout
    m2, _ = _tiny()
    m2.load_state_dict(msd)
    o2 = FusedAdam(m2.parameters(), lr=1e-3, model=m2)
    o2.load_state_dict(sd)
    run(m2, o2, 2, 20)
    # not bit-exact: the backward kernels use float atomics (order varies run to run), and Adam turns the rounding noise
    # of the analytically-zero k_proj.bias gradient into +-lr steps -- those entries are excluded
    p1 = dict(model.named_parameters())

    def same_params(m):
        for n, p in m.named_parameters():
            if n.endswith("k_proj.bias"):
                continue
            assert (p.detach() - p1[n].detach()).abs().max().item() <= 2e-5 * max(p1[n].abs().max().item(), 1e-3), n

    same_params(m2)
    assert o2.step_count == opt.step_count == 4
    # different layout: no packed q|k|v groups
    m3, _ = _tiny()
    m3.load_state_dict(msd)
    o3 = FusedAdam(m3.parameters(), lr=1e-3, pack=False)
    assert o3._layout() != opt._layout()
    with pytest.raises(ValueError):
        o3.load_state_dict(sd)
    o3.load_state_dict(sd, names=names)
    run(m3, o3, 2, 20)
    same_params(m3)
    # fairseq-shaped state
    fsd = opt.fairseq_state_dict()
    assert set(fsd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and fsd["state"][0]["exp_avg"].shape == opt.params[0].shape
    o4 = FusedAdam(_tiny()[0].parameters(), lr=1e-3)
    o4.load_fairseq_state_dict(fsd)
    for i, (p, o) in enumerate(zip(o4.params, o4.offsets)):
        assert torch.equal(o4.exp_avg[o:o + p.numel()].view(p.shape), fsd["state"][i]["exp_avg"])


def test_downstream_consumer_call_patterns():
    """The two consumers SURVEY.md 8(f) rank 4 names, called the way the reference's own code calls them:
    (a) s3prl's UpstreamExpert (downstreams/speaker_verification/models/utils.py:49-75): forward hooks on
        model.encoder.layers[i] reading `input[0].transpose(0, 1)` and on model.encoder reading `output[0]`, then
        model.extract_features(padded_wav, padding_mask=mask, mask=None);
    (b) the k-means feature dump (src/examples/hubert/simple_kmeans/dump_hubert_feature.py:68-80):
        model.extract_features(source=chunk, padding_mask=None, mask=False, output_layer=L) in chunks.
    Checked against the CPU oracle's layer inputs / outputs (tiny golden weights)."""
    from conftest import Cfg
    from oracle import wavlm_oracle as O
    model, z = _tiny()
    model.eval()
    sd = golden_state_dict(z)
    cfg = Cfg(**TINY)
    wavs = [torch.from_numpy(z["in/source"][0]), torch.from_numpy(z["in/source"][1][:12000])]
    # ---- (a)
    got = []
    handles = [l.register_forward_hook(lambda m, inp, out: got.append(inp[0].transpose(0, 1))) for l in model.encoder.layers]
    handles.append(model.encoder.register_forward_hook(lambda m, inp, out: got.append(out[0])))
    lengths = torch.LongTensor([len(w) for w in wavs])
    pmask = ~torch.lt(torch.arange(int(lengths.max())).unsqueeze(0), lengths.unsqueeze(1))
    padded = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True)
    with torch.no_grad():
        feats, fpm = model.extract_features(padded.cuda(), padding_mask=pmask.cuda(), mask=None)
    for h in handles:
        h.remove()
    ref = O.extract_features(sd, cfg, padded, padding_mask=pmask, output_layer=cfg.encoder_layers)
    want = [t.transpose(0, 1) for t, _ in ref["layer_results"][:cfg.encoder_layers]] + [ref["x"]]
    assert len(got) == len(want) == cfg.encoder_layers + 1
    for a, b in zip(got, want):
        assert a.shape == b.shape
        assert ((a.cpu() - b).abs().max() / b.abs().max()).item() < 1e-4
    assert ((feats.cpu() - ref["x"]).abs().max() / ref["x"].abs().max()).item() < 1e-4
    assert torch.equal(fpm.cpu(), ref["padding_mask"])
    # ---- (b)
    x = wavs[0].view(1, -1)
    with torch.no_grad():
        chunks = [model.extract_features(source=x[:, s:s + 8000].cuda(), padding_mask=None, mask=False, output_layer=1)[0]
                  for s in range(0, x.size(1), 8000)]
        feat = torch.cat(chunks, 1).squeeze(0)
    refc = torch.cat([O.extract_features(sd, cfg, x[:, s:s + 8000], output_layer=1)["x"] for s in range(0, x.size(1), 8000)], 1)
    assert ((feat.cpu() - refc.squeeze(0)).abs().max() / refc.abs().max()).item() < 1e-4


# ------------------------------------------------------------------------------------------------ RCCL, world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _nccl_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if world == 1:
        os.environ["WAVLM_DP_FORCE"] = "1"   # a one-rank group runs the whole machinery (bench.py --force-dp)
    import torch.distributed as dist
    try:
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
        import unispeech_amd.functional as F
        from unispeech_amd.dp import DataParallelWavLM
        from unispeech_amd.optim import FusedAdam
        from unispeech_amd.pretrain import WavLMCriterion, WavLMPretrainConfig, WavLMPretrainModel
        from test_model_gpu import BASE
        d = dict(BASE)
        d.update(encoder_layers=3)
        cfg = WavLMPretrainConfig(**{k: v for k, v in d.items() if k in WavLMPretrainConfig.__dataclass_fields__})
        torch.manual_seed(0)
        model = WavLMPretrainModel(cfg, None, [range(104)]).cuda().to(torch.bfloat16).train()
        crit = WavLMCriterion(None, 1.0, 0.0, loss_weights=[10.0], defer_logging=True)
        opt = FusedAdam(model.parameters(), model=model)
        dp = DataParallelWavLM(model, opt, bucket_bytes=4 << 20)
        assert dp.reducer.enabled and dp.reducer.comm_stream is not None and len(dp.reducer.buckets) >= 2
        B, T = 2, 24000
        g = torch.Generator().manual_seed(100 + rank)
        wav = torch.randn(B, T, generator=g).cuda().to(torch.bfloat16)
        target = torch.randint(4, 104, (B, 75), generator=g).cuda()
        sample = {"id": torch.arange(B), "net_input": {"source": wav, "padding_mask": torch.zeros(B, T, dtype=torch.bool).cuda()},
                  "target_list": [target]}

        def backward():
            np.random.seed(11 + rank)
            torch.manual_seed(5)
            F._SEED_CTR[0] = 0
            loss, _, _ = crit(dp, sample)
            loss.backward()

        opt.zero_grad()
        with dp.no_sync():
            backward()
        local = opt.flat_grad.detach().float().clone()
        gathered = [torch.zeros_like(local) for _ in range(world)]
        dist.all_gather(gathered, local)
        want = sum(gathered)
        opt.zero_grad()
        backward()
        early = sum(dp.reducer._launched)
        dp.all_reduce_grads()
        torch.cuda.synchronize()
        got = opt.flat_grad.detach().float()
        err = ((got - want).abs().max() / want.abs().max().clamp_min(1e-6)).item()
        q.put((rank, err, early, len(dp.reducer.buckets), None))
    except Exception:
        import traceback
        q.put((rank, float("inf"), 0, 0, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.gpu
def test_dp_world2_rccl_gradients_sum_over_ranks():
    """the real transport: one rank per GPU, backend nccl (= RCCL), bucket all-reduces on the side stream while backward
    runs; the reduced arena must equal the sum of the ranks' local gradients.  Two ranks where two GPUs are visible.  RCCL
    refuses two ranks on one device, so with one GPU the same worker runs as a one-rank RCCL group with the machinery
    forced on (WAVLM_DP_FORCE=1, as `bench.py --force-dp`): the buckets still go through RCCL on the side stream while
    backward runs, and the arena must come back equal to the rank's own gradient (the sum over two ranks on one GPU is
    tests/test_dp_gpu.py, over gloo)."""
    import torch.multiprocessing as mp
    world = min(2, torch.cuda.device_count())
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_nccl_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, err, early, nb, tb in res:
        assert tb is None, tb
        assert err < 1e-2, (rank, err)
        assert early >= nb // 2


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])
def test_preln_fused_residuals_match_the_unfused_blocks(dtype, tol):
    """Pre-LN encoder (WavLM-Large structure): the training path that fuses both residual adds of a block into the
    LayerNorm that follows them (forward_preln_fused; the LayerNorm backward also delivers the out_proj / fc2 bias
    gradients) against the block-by-block form, same weights and input, dropout 0: output and every gradient."""
    from unispeech_amd import wavlm as W
    from unispeech_amd.wavlm import WavLM, WavLMConfig
    d = dict(encoder_layers=3, encoder_embed_dim=256, encoder_ffn_embed_dim=512, encoder_attention_heads=4,
             conv_feature_layers="[(64,10,5)] + [(64,3,2)] * 2", extractor_mode="layer_norm", layer_norm_first=True,
             normalize=True, conv_bias=True, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0,
             encoder_layerdrop=0.0, relative_position_embedding=True, gru_rel_pos=True, num_buckets=32, max_distance=64,
             conv_pos=16, conv_pos_groups=4)
    torch.manual_seed(3)
    m = WavLM(WavLMConfig(d)).cuda().to(dtype).train()
    wav = torch.randn(2, 8000, device="cuda").to(dtype)
    probe = None
    res = []
    for fused in (True, False):
        W.PRELN_FUSED = fused
        try:
            m.zero_grad(set_to_none=True)
            np.random.seed(1)
            x, _ = m.extract_features(wav)
            if probe is None:
                probe = torch.randn_like(x)
            (x.float() * probe.float()).sum().backward()
            res.append((x.detach().float().clone(), {n: p.grad.detach().float().clone() for n, p in m.named_parameters()
                                                      if p.grad is not None}))
        finally:
            W.PRELN_FUSED = True
    (xa, ga), (xb, gb) = res
    assert ((xa - xb).abs().max() / xb.abs().max()).item() < tol
    assert ga.keys() == gb.keys()
    gmax = max(v.abs().max().item() for v in gb.values())
    for n in ga:
        scale = max(gb[n].abs().max().item(), 1e-3 * gmax)
        assert ((ga[n] - gb[n]).abs().max().item() / scale) < tol, n


@pytest.mark.gpu
def test_preln_fused_speaker_tap_when_the_tap_layer_is_dropped():
    """UniSpeech-SAT Large structure under layerdrop: the speaker tap is the residual stream after the last block that RAN
    before (or at) the tap layer (unispeech_sat.py:1238-1247 records `x` after the layerdrop branch).  In the fused pre-LN
    path that block's feed-forward output is still pending when the tap layer is skipped: tap, output and gradients must
    equal the block-by-block form for a draw that drops the tap layer."""
    from types import SimpleNamespace
    from unispeech_amd import wavlm as W
    from unispeech_amd.wavlm import TransformerEncoder
    args = SimpleNamespace(dropout=0.0, encoder_embed_dim=128, conv_pos=16, conv_pos_groups=4, relative_position_embedding=True,
                           num_buckets=32, max_distance=64, gru_rel_pos=True, encoder_ffn_embed_dim=256,
                           encoder_attention_heads=2, attention_dropout=0.0, activation_dropout=0.0, activation_fn="gelu",
                           layer_norm_first=True, encoder_layers=4, encoder_layerdrop=0.5, utterance_contrastive_loss=True)
    torch.manual_seed(5)
    enc = TransformerEncoder(args).cuda().train()
    x0 = torch.randn(2, 40, 128, device="cuda")
    tap = 2
    seed = None
    for s in range(200):  # a draw that runs layers 0 and 1, drops the tap layer, runs layer 3 (one host draw per layer)
        np.random.seed(s)
        d = [np.random.random() > args.encoder_layerdrop for _ in range(4)]
        if d == [True, True, False, True]:
            seed = s
            break
    assert seed is not None
    res = []
    probe = None
    for fused in (True, False):
        W.PRELN_FUSED = fused
        try:
            enc.zero_grad(set_to_none=True)
            np.random.seed(seed)
            x, _, _, er = enc(x0, extract_layer=tap)
            if probe is None:
                probe = (torch.randn_like(x), torch.randn_like(er))
            ((x * probe[0]).sum() + (er * probe[1]).sum()).backward()
            res.append((x.detach().clone(), er.detach().clone(),
                        {n: p.grad.detach().clone() for n, p in enc.named_parameters() if p.grad is not None}))
        finally:
            W.PRELN_FUSED = True
    (xa, ea, ga), (xb, eb, gb) = res
    assert ((xa - xb).abs().max() / xb.abs().max()).item() < 2e-5
    assert ((ea - eb).abs().max() / eb.abs().max()).item() < 2e-5
    assert ga.keys() == gb.keys()
    gmax = max(v.abs().max().item() for v in gb.values())
    for n in ga:
        scale = max(gb[n].abs().max().item(), 1e-3 * gmax)
        assert ((ga[n] - gb[n]).abs().max().item() / scale) < 5e-5, n
    assert any(n.startswith("layers.1.fc2") for n in ga) and not any(n.startswith("layers.2.") for n in ga)


@pytest.mark.gpu
def test_sat_large_remove_pretraining_modules_then_features_only():
    """fine-tuning / feature extraction after remove_pretraining_modules() on a pre-LN SAT model: the speaker tap is no
    longer requested (unispeech_sat.py:828-834), so forward(features_only=True) works without layer_norm_for_extract"""
    from unispeech_amd.pretrain import WavLMPretrainConfig, WavLMPretrainModel
    from conftest import TINY
    d = dict(TINY)
    d.update(layer_norm_first=True, extractor_mode="layer_norm", utterance_contrastive_loss=True, utterance_contrastive_layer=1)
    cfg = WavLMPretrainConfig(**{k: v for k, v in d.items() if k in WavLMPretrainConfig.__dataclass_fields__})
    torch.manual_seed(0)
    m = WavLMPretrainModel(cfg, None, [range(23)]).cuda().eval()
    m.remove_pretraining_modules()
    assert m.utterance_contrastive_loss is False and m.utterance_contrastive_layer is None
    wav = torch.randn(2, 4000, device="cuda")
    with torch.no_grad():
        out = m(wav, padding_mask=torch.zeros(2, 4000, dtype=torch.bool, device="cuda"), mask=False, features_only=True)
    assert torch.isfinite(out["x"]).all()


@pytest.mark.gpu
def test_bench_four_ranks_on_one_gpu_over_gloo():
    """`bench.py --gpus 4` end to end with every rank on cuda:0 and gloo as the transport (WAVLM_SHARED_GPU=1,
    WAVLM_DIST_BACKEND=gloo): the self-launch under torch.distributed.run, the rank-count check, four reducers issuing
    their buckets in the same order, the Trainer-order step (average, then world / sample_size) and the max-over-ranks
    timing all run with more than two ranks.  Four, not the eight of a node: every rank opens the one GPU, and with this
    process that stays within six processes on one GPU at a time.  Tiny batch; the numbers mean nothing, the line must be
    sane."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WAVLM_SHARED_GPU="1", WAVLM_DIST_BACKEND="gloo")
    # (--dp-alt-pass never: the alternative pass would start one more process per rank on the same GPU; the two-rank test
    # below covers it)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "4", "--batch", "1", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--no-roofline", "--dp-alt-pass", "never"], cwd=root, env=env, capture_output=True,
                       text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line from rank 0: " + r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4 and out["config"]["parallelism"] == "dp4" and out["config"]["global_batch"] == 4
    assert out["ranks_seen"] == 4 and out["distinct_devices"] == 1 and out["dist_backend"] == "gloo"
    assert out["scaling"] == "weak" and out["value"] > 0 and np.isfinite(out["final_loss"])


@pytest.mark.gpu
def test_bench_data_parallel_self_diagnosis_and_alternative_pass():
    """The first run on a real multi-GPU node has to explain itself: `bench.py --gpus 2 --full` prints, per
    gradient bucket, when its all-reduce was launched relative to the end of backward, how long it took, its bus bandwidth
    and what the last bucket leaves exposed -- and (here forced with --dp-alt-pass always, on a node: whenever a rank waits
    > 1 ms) repeats the measurement in fresh processes with NCCL_MAX_NCHANNELS unset and no CUs reserved, printing both in
    ONE line.  Two ranks on one GPU over gloo: the mechanics are the same, the numbers mean nothing."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WAVLM_SHARED_GPU="1", WAVLM_DIST_BACKEND="gloo", WAVLM_DP_BUCKET_MIB="32")
    env.pop("NCCL_MAX_NCHANNELS", None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--batch", "1", "--steps", "2", "--warmup", "1", "--full",
                        "--no-cpu-baseline", "--no-roofline", "--dp-alt-pass", "always"], cwd=root, env=env, capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line from rank 0: " + r.stdout[-2000:]
    dp = json.loads(lines[0])["data_parallel"]
    rows = dp["buckets_rank0"]
    assert rows and [r_["bucket"] for r_ in rows] == list(range(dp["buckets"]))
    assert abs(sum(r_["mib"] for r_ in rows) - dp["grad_arena_mib"]) < 0.2 * len(rows) + 0.5   # the buckets tile the arena
    assert all(r_["allreduce_ms"] > 0 and r_["bus_gb_s"] > 0 for r_ in rows)
    assert dp["exposed_ms_last_bucket_rank0"] >= 0 and dp["allreduce_bus_gb_s_rank0"] > 0
    assert dp["rccl_max_nchannels"] == "6" and dp["reserved_cus"] == 6           # the default configuration is the headline
    alt = dp["alt_pass"]
    assert "error" not in alt, alt
    assert alt["settings"] == {"NCCL_MAX_NCHANNELS": None, "WAVLM_DP_RESERVED_CUS": 0}
    assert alt["value"] > 0 and len(alt["comm_wait_ms_per_rank"]) == 2 and alt["buckets_rank0"]
    assert isinstance(dp["alt_pass_faster_than_default"], bool)
    assert dp.get("alt_pass_native") is None     # the native-transport pass needs RCCL with one device per rank (a node)
    top = json.loads(lines[0])
    assert top["ranks_seen"] == 2 and top["distinct_devices"] == 1 and top["dist_backend"] == "gloo" and top["dp_transport"] == "torch"


@pytest.mark.gpu
def test_bench_force_dp_prices_the_data_parallel_machinery_on_one_gpu():
    """what the N > 1 path costs a rank BEFORE any byte crosses a link, measurable on one GPU.
    `bench.py --force-dp` runs the headline step through DataParallelWavLM over a ONE-rank RCCL group: arena buckets
    all-reduced on the side stream as backward produces them (an in-place copy kernel at world 1), gradient listeners, six CUs
    reserved in every persistent GEMM grid, NCCL_MAX_NCHANNELS capped, the sample-size all-reduce.  Its ms_per_step must stay
    within 4 % of the plain `--gpus 1` path on the same box (the reservation alone was measured at +0.5 %,
    profiles/r04/reserved_cus_*.txt; run-to-run noise of two short runs ~1 %), the loss must be the same number, and the line
    of --full carries the `data_parallel` block a node run prints."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("NCCL_MAX_NCHANNELS", "WAVLM_DP_FORCE", "WAVLM_SHARED_GPU", "WAVLM_DIST_BACKEND"):
        env.pop(k, None)
    out = {}
    for tag, extra in (("plain", []), ("dp", ["--force-dp"])):
        r = subprocess.run([sys.executable, "bench.py", "--steps", "10", "--warmup", "3", "--full", "--no-cpu-baseline",
                            "--no-roofline", "--no-secondary", "--no-busy", "--no-settle"] + extra, cwd=root, env=env,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out[tag] = json.loads(lines[0])
    a, b = out["plain"], out["dp"]
    dp = b["data_parallel"]
    print("plain %.2f ms/step, through the data-parallel machinery %.2f ms/step (%+.1f %%); buckets %d, reserved CUs %d, channels %s, "
          "comm wait %s ms" % (a["ms_per_step"], b["ms_per_step"], 100.0 * (b["ms_per_step"] / a["ms_per_step"] - 1.0), dp["buckets"],
                               dp["reserved_cus"], dp["rccl_max_nchannels"], dp["comm_wait_ms_per_rank"]))
    assert "data_parallel" not in a
    assert dp["ranks_seen"] == 1 and dp["backend"] == "nccl" and dp["transport"] == "torch"
    assert dp["buckets"] >= 4 and dp["reserved_cus"] == 6 and dp["rccl_max_nchannels"] == "6"
    assert dp["buckets_rank0"] and all(r_["allreduce_ms"] > 0 for r_ in dp["buckets_rank0"])
    assert abs(a["final_loss"] - b["final_loss"]) <= 2e-3 * abs(a["final_loss"])   # same seeds, same step: sums of one rank
    assert b["ms_per_step"] <= 1.04 * a["ms_per_step"], (a["ms_per_step"], b["ms_per_step"])


@pytest.mark.gpu
def test_bench_plain_run_prints_the_headline_only():
    """A plain `bench.py --gpus 1` run sets up, warms up, settles, times its steps and prints the line: nothing that
    `--full` adds (ms_per_step_unsettled, gpu_busy / host_enqueue, roofline, cpu_baseline, secondary) is in it, and the
    headline fields are all there."""
    import json
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    steps, warmup = 3, 2
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=root,
                       capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    print("plain run: %.1f s of wall, %.1f s outside the warm-up and timed steps" % (wall, wall - (steps + warmup) * out["ms_per_step"] / 1e3))
    assert out["steps"] == steps and out["warmup"] == warmup and out["n_gpus"] == 1
    assert out["unit"] == "audio-s/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["ms_per_step"] > 0 and out["value"] > 0 and out["settle_steps"] >= 1
    assert out["gpu_busy_ms_per_step"] is None and out["host_enqueue_ms_per_step"] is None and out["ms_per_step_unsettled"] is None
    assert not {"roofline", "cpu_baseline", "secondary", "data_parallel"} & set(out)
