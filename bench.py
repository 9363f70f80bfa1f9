#!/usr/bin/env python
"""Headline benchmark: WavLM-Base pre-training throughput in audio-seconds/sec (BASELINE.json metric), config[1]:
bf16, 32 x 15 s utterances per GPU, masked-prediction loss, forward + backward + gradient reduction + fused Adam.

    python bench.py --gpus 1 --steps K --warmup W
    python bench.py --gpus 1 --steps K --warmup W --full   # the same headline + every diagnostic leg (below)
    python bench.py --gpus N ...                        # no launcher: re-executes itself under torch.distributed.run
    python bench.py --config large ...                  # WavLM-Large, 20 s utterances (configs[3] per-GPU slice)
    python bench.py --config extract ...                # eval `extract_features` per call, 32 x 15 s
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W          # one rank per GPU over RCCL, weak scaling

Synthetic data of the real shape (randn waveform, random k-means labels), random-init weights of the real
architecture; recipe dropouts on (dropout 0.1, attention_dropout 0.1, dropout_input 0.1), layerdrop 0 (no layer is
ever skipped inside the timed region).  Rank 0 prints ONE JSON line.

A plain run does what the headline needs and nothing else: set-up, W warm-up steps, the untimed settling steps (K steps,
then until two consecutive steps agree), the K timed steps, `--dump-outputs` if given, the line. `--full` adds every
other leg, all outside the timed region: `ms_per_step_unsettled` (the time of the first K settling steps),
`gpu_busy_ms_per_step` / `host_enqueue_ms_per_step`, `roofline` (HIP-event timing of every bf16 MFMA GEMM launch during
extra steps; `roofline.kernels` carries the same live measurement for the fused attention forward / backward
(MFMA-bound), the conv0 stage and the LayerNorm row kernels (HBM-bound)), `cpu_baseline` (the CPU oracle timed on the
host cores on a bounded 1 x 15 s sample, thread count chosen by a sweep on the sample itself; rank 0, N=1 only),
`secondary` (config base, N=1) and, for data-parallel runs, the `data_parallel` block with its alternative passes. The
`--no-*` switches take single legs out of a `--full` run.
"""
import argparse
import json
import os
import sys
import time

# the host driver only supports dmabuf IPC: without this RCCL / cross-process device memory sharing fails with
# `hipIpcGetMemHandle: invalid argument` (set before torch / HIP initialise; a no-op when the launcher exported it)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SECONDS = 15.0
SR = 16000
BATCH_PER_GPU = 32
V = 504
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense, /opt/skills/guides/MI355X_MICROARCH.md line 42
HBM_PEAK_GBS = 8000.0           # HBM3E spec, ibid. line 35 (the guide measures 6.29 TB/s on a copy)


# name -> (layers, d, ffn, heads, extractor_mode, layer_norm_first, seconds, label); "base" is BASELINE.json configs[1]
# (the headline), "large" the per-GPU slice of configs[3] (WavLM-Large, 20 s utterances)
CONFIGS = {
    "base": dict(L=12, D=768, F=3072, H=12, mode="default", pre_ln=False, seconds=15.0,
                 name="WavLM-Base (12L, d=768)", baseline="BASELINE.json configs[1]", fgm=0.1),
    "large": dict(L=24, D=1024, F=4096, H=16, mode="layer_norm", pre_ln=True, seconds=20.0,
                  name="WavLM-Large (24L, d=1024)", baseline="per-GPU slice of BASELINE.json configs[3]", fgm=1.0),
    # configs[4]: UniSpeech-SAT Large = the Large structure + utterance mixing of the batch (task defaults: mixing_prob 0.5,
    # mixing_num 1, utterance_mixing_pretraining.py:103-114) + the utterance-contrastive head on layer 6 (model defaults:
    # unispeech_sat.py:248-262).  The mixing kernel runs INSIDE the timed step (the un-mixed collated batch is resident).
    "sat_large": dict(L=24, D=1024, F=4096, H=16, mode="layer_norm", pre_ln=True, seconds=20.0,
                      name="UniSpeech-SAT Large (24L, d=1024, utterance mixing + contrastive head)",
                      baseline="per-GPU slice of BASELINE.json configs[4]", fgm=1.0, sat=True),
    # the metric "per call for extract_features" -- the standalone WavLM.extract_features API
    # (WavLM/WavLM.py:323-375), eval mode, no mask, no padding mask, bf16, the batch of configs[1]
    "extract": dict(L=12, D=768, F=3072, H=12, mode="default", pre_ln=False, seconds=15.0,
                    name="WavLM-Base (12L, d=768)", baseline="the batch of BASELINE.json configs[1], forward API of configs[0]",
                    fgm=0.1, extract=True),
}


def base_cfg(training_dropouts=True, config="base"):
    from unispeech_amd.pretrain import WavLMPretrainConfig
    c = CONFIGS[config]
    d = 0.1 if training_dropouts else 0.0
    return WavLMPretrainConfig(
        encoder_layers=c["L"], encoder_embed_dim=c["D"], encoder_ffn_embed_dim=c["F"], encoder_attention_heads=c["H"],
        dropout=d, attention_dropout=d, activation_dropout=0.0, encoder_layerdrop=0.0, dropout_input=d,
        dropout_features=d, feature_grad_mult=c["fgm"], mask_prob=0.80, mask_length=10, final_dim=256 if config == "base" else 768,
        logit_temp=0.1, relative_position_embedding=True, num_buckets=320, max_distance=800, gru_rel_pos=True,
        label_rate=50, extractor_mode=c["mode"], layer_norm_first=c["pre_ln"],
        utterance_contrastive_loss=bool(c.get("sat")), utterance_contrastive_layer=6, num_instances=0, cross_sample_instances=100,
        conv_feature_layers="[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2")


def algorithmic_flops_per_step(B, T, config="base"):
    """forward FLOPs of the model for B utterances of T samples, x3 for forward+backward"""
    c = CONFIGS[config]
    fl = 0.0
    t, cin = T, 1
    for (co, k, s) in [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2:
        t = (t - k) // s + 1
        fl += 2.0 * B * t * co * cin * k
        cin = co
    n, D, Fd, H = B * t, c["D"], c["F"], c["H"]
    fl += 2.0 * n * 512 * D                      # post_extract_proj
    fl += 2.0 * n * D * (D // 16) * 128          # pos_conv
    per_layer = 2.0 * n * D * D * 4 + 2.0 * n * D * Fd * 2 + 2.0 * B * H * t * t * (D // H) * 2
    fl += c["L"] * per_layer
    return 3.0 * fl


def cpu_baseline():
    """reference algorithm (CPU oracle = PyTorch fp32 on the host cores) on a bounded sample of the same workload:
    forward + loss + backward of ONE 15 s utterance through the 12-layer model, 1 warm-up + 3 timed iterations, median.
    The thread count comes from a sweep on the 15 s sample itself (_pick_threads) and is stated in `cores`."""
    from oracle import wavlm_oracle as O
    from unispeech_amd.masking import compute_mask_indices
    from unispeech_amd.pretrain import WavLMPretrainModel
    cfg = base_cfg(False)
    torch.manual_seed(0)
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point())
          for k, v in WavLMPretrainModel(cfg, None, [range(V)]).state_dict().items()}

    def run(seconds, seed):
        B, T = 1, int(seconds * SR)
        g = torch.Generator().manual_seed(seed)
        wav = torch.randn(B, T, generator=g)
        Tp = T
        for k, s_ in [(10, 5)] + [(3, 2)] * 4 + [(2, 2)] * 2:
            Tp = (Tp - k) // s_ + 1
        target = torch.randint(4, V, (B, max(int(50 * seconds), Tp)), generator=g)
        pm = torch.zeros(B, T, dtype=torch.bool)
        np.random.seed(123)
        mask = torch.from_numpy(compute_mask_indices((B, Tp), torch.zeros(B, Tp, dtype=torch.bool), cfg.mask_prob,
                                                     cfg.mask_length, "static", 0, min_masks=2))
        for p in sd.values():
            p.grad = None
        t0 = time.time()
        net = O.pretrain_forward(sd, cfg, wav, [target], pm, mask, [V])
        loss, _, _ = O.criterion(net, 1.0, 0.0, [10.0])
        loss.backward()
        return time.time() - t0

    from unispeech_amd import hostenv
    ncpu = hostenv.usable_cpus()   # cores the container may actually use (cgroup quota: 16 of the GPU box's 256)
    # never the full core count of a big host: 256 OpenMP threads on these many small ops ran a 3 s probe in 170 s
    # (against 0.45 s on 8 threads) on the GPU box -- the container is throttled to its quota
    best, sweep = _pick_threads(lambda: run(SECONDS, 2), ncpu)
    old = torch.get_num_threads()
    torch.set_num_threads(best)
    times = sorted(run(SECONDS, 2) for _ in range(3))
    torch.set_num_threads(old)
    return {"value": round(SECONDS / times[1], 2), "unit": "audio-s/s", "cores": best, "kind": "port",
            "sample": "oracle fwd+loss+bwd fp32, 12 layers, B=1 x 15 s, median of 3 after 1 warm-up; threads swept ON THE 15 s "
                      "SAMPLE ITSELF (seconds per run: %s; the largest count within 5 %% of the fastest is used; host has %d usable "
                      "CPUs).  kind = port: the GPU box has no /root/reference; the reference's own WavLMModel + WavLMCriterion timed beside "
                      "this oracle on one host (same threads, same 15 s sample, identical loss): 3.2-4.9 s against 3.8 s per run -- "
                      "profiles/r06/ref_vs_oracle_cpu.txt" % ({c: round(t, 2) for c, t in sweep.items()}, ncpu)}


def _pick_threads(run_once, ncpu):
    """thread count for a cpu_baseline leg: one warm-up, then one run of the SAMPLE ITSELF per candidate count (round 4 swept on
    a 3 s utterance where 4 / 8 / 16 threads differed by noise, and the 15 s sample then ran on 4 of 16 CPUs: VERDICT r4 weak
    6).  Returns (the LARGEST candidate within 5 % of the fastest, {threads: seconds}) -- a difference below 5 % is noise and
    SURVEY 8(d) asks for all usable cores."""
    cands = sorted({c for c in (4, 8, 16, 32) if c <= ncpu} | ({ncpu} if ncpu <= 32 else set())) or [1]
    old = torch.get_num_threads()
    torch.set_num_threads(cands[-1])
    run_once()  # warm-up (allocator, oneDNN primitive caches)
    sweep = {}
    for c in cands:
        torch.set_num_threads(c)
        sweep[c] = run_once()
    torch.set_num_threads(old)
    fastest = min(sweep.values())
    best = max(c for c, t in sweep.items() if t <= 1.05 * fastest)
    return best, sweep


def cpu_baseline_extract():
    """the oracle's `extract_features` (eval, no mask) on ONE 15 s utterance, fp32 on the host cores: BASELINE.json
    configs[0]'s CPU-runnable case scaled to one utterance; threads by the same sweep as cpu_baseline()"""
    from oracle import wavlm_oracle as O
    from unispeech_amd.wavlm import WavLM, WavLMConfig
    cfg = extract_cfg()
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in WavLM(cfg).state_dict().items()}

    def run(seconds, seed):
        wav = torch.randn(1, int(seconds * SR), generator=torch.Generator().manual_seed(seed))
        t0 = time.time()
        with torch.no_grad():
            O.extract_features(sd, cfg, wav)
        return time.time() - t0

    from unispeech_amd import hostenv
    ncpu = hostenv.usable_cpus()
    best, sweep = _pick_threads(lambda: run(SECONDS, 2), ncpu)
    old = torch.get_num_threads()
    torch.set_num_threads(best)
    times = sorted(run(SECONDS, 2) for _ in range(5))
    torch.set_num_threads(old)
    return {"value": round(SECONDS / times[2], 2), "unit": "audio-s/s", "cores": best, "kind": "port",
            "sample": "oracle extract_features fp32 eval, 12 layers, B=1 x 15 s, median of 5 after 1 warm-up; threads swept on the "
                      "15 s sample itself (seconds per run: %s; the largest count within 5 %% of the fastest; host has %d usable "
                      "CPUs)" % ({c: round(t, 2) for c, t in sweep.items()}, ncpu)}


def extract_cfg():
    from unispeech_amd.wavlm import WavLMConfig
    return WavLMConfig(dict(encoder_layers=12, encoder_embed_dim=768, encoder_ffn_embed_dim=3072, encoder_attention_heads=12,
                            relative_position_embedding=True, num_buckets=320, max_distance=800, gru_rel_pos=True,
                            feature_grad_mult=0.1, mask_prob=0.8))


def kernel_rooflines(ops, nsteps):
    """per-kernel-class roofline entries from the HIP events of the profiled steps (the same live measurement as the GEMM
    entry): attention against the MFMA peak, conv0 / LayerNorm against the HBM peak"""
    out = []
    for name, bound, what in (
            ("attn_fwd", "mfma", "fused gated-relative-position attention forward (attn_fwd_kernel): 4 B H T^2 hd FLOPs per call"),
            ("attn_bwd", "mfma", "fused attention backward (attn_bwd_dq_kernel + attn_bwd_dkv_kernel + finishing launches): 10 B H T^2 hd FLOPs per call"),
            ("conv0_fwd", "hbm", "conv0 + norm + GELU forward stage: waveform read once, output written once"),
            ("conv0_bwd", "hbm", "conv0 stage backward: the incoming gradient read once (+ waveform)"),
            ("ln_fwd", "hbm", "LayerNorm (+ residual / dropout / GELU) forward row kernel: every input / output tensor once"),
            ("ln_bwd", "hbm", "LayerNorm backward row kernel + parameter-gradient finish: every input / output tensor once")):
        n, ms, fl, by = ops.prof_collect_class(name)
        if n == 0 or ms <= 0:
            continue
        if bound == "mfma":
            ach = fl / (ms * 1e-3) / 1e12
            e = {"achieved": round(ach, 1), "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / BF16_MFMA_PEAK_TFLOPS, 4)}
        else:
            ach = by / (ms * 1e-3) / 1e9
            e = {"achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4)}
        e.update(name=name, bound=bound, kernel=what, calls_per_step=n // nsteps, ms_per_step=round(ms / nsteps, 3),
                 avg_call_us=round(ms / n * 1e3, 2), algorithmic_bytes_per_call=round(by / n))
        out.append(e)
    return out


def live_gemm_traffic(args):
    """(HBM bytes per GEMM launch, source string, GEMM launches per step seen by the counters) from two rocprofv3 PMC passes
    of this command run as subprocesses, or (None, None, None) when rocprofv3 is missing / a pass fails / times out.  Same
    reduction as tools/pmc_traffic.py: EVERY kernel whose name starts with `gemm_` (round 4's name list missed
    gemm_w4_kernel); the split-K reductions' bytes count, their launches do not (they belong to their GEMM's launch)."""
    import collections
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, None, None
    tmp = tempfile.mkdtemp(prefix="wavlm_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    tot = {}
    launches = 0
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, ctr)
            cmd = [exe, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "run", "--", sys.executable,
                   os.path.abspath(__file__), "--steps", "1", "--warmup", "1", "--no-settle",   # a plain run: no other leg
                   "--config", args.config, "--batch", str(args.batch)]
            r = subprocess.run(cmd, env=env, cwd="/tmp", capture_output=True, text=True, timeout=300)
            files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return None, None, None
            per = collections.defaultdict(lambda: [0, 0.0])
            for row in csv.DictReader(open(files[0])):
                if row["Counter_Name"] != ctr:
                    continue
                name = row["Kernel_Name"].split("(")[0].replace("void ", "")
                if name.startswith("gemm_"):
                    per[name][0] += 1
                    per[name][1] += float(row["Counter_Value"])
            scale = 2.0 * 1024.0 if ctr == "FETCH_SIZE" else 1024.0   # gfx950: FETCH_SIZE counts 128-B requests as 64 B
            launches = sum(v[0] for k, v in per.items() if not k.startswith("gemm_splitk"))
            if launches == 0:
                return None, None, None
            tot[ctr] = sum(v[1] for v in per.values()) * scale / launches   # per launch of THIS pass
        # each pass runs 1 warm-up + 1 timed step of the same launch sequence
        return round(tot["FETCH_SIZE"] + tot["WRITE_SIZE"]), \
            "live: two rocprofv3 --pmc passes (FETCH_SIZE x 2, WRITE_SIZE) of this command, 2 steps each, %d GEMM launches" % launches, \
            launches / 2.0
    except Exception:
        return None, None, None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def secondary_lines(configs=("large", "extract"), steps=5, warmup=2):
    """{config: {ms_per_step, value, unit, frac, ...}}: `bench.py --config <c> --steps 5 --warmup 2 --full` without its CPU
    baseline and clocks legs, in a fresh process each (a crash or time-out there is reported under the config's name and
    cannot take the headline down)"""
    import subprocess
    res = {}
    for c in configs:
        cmd = [sys.executable, os.path.abspath(__file__), "--config", c, "--steps", str(steps), "--warmup", str(warmup),
               "--full", "--no-cpu-baseline", "--no-busy", "--no-secondary"]
        t0 = time.time()
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
            line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), None)
            if line is None:
                res[c] = {"error": "no result line (rc %d): %s" % (r.returncode, r.stderr[-300:])}
                continue
            d = json.loads(line)
            roof = d.get("roofline") or {}
            res[c] = {"metric": d["metric"], "value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"],
                      "steps": d["steps"], "warmup": d["warmup"], "settle_steps": d.get("settle_steps"), "dtype": d["dtype"],
                      "workload": d["config"]["workload"], "model_tflops": d.get("model_tflops"),
                      "frac": roof.get("frac"), "gemm_ms_per_step": roof.get("gemm_ms_per_step"),
                      "kernels": [{k: e.get(k) for k in ("name", "frac", "avg_call_us", "ms_per_step")} for e in roof.get("kernels", [])],
                      "wall_s": round(time.time() - t0, 1)}
        except Exception as e:   # noqa: BLE001 -- a side leg must not take the headline down
            res[c] = {"error": "%s: %s" % (type(e).__name__, e)}
    return res


def pin_rank_cores(local_rank, local_world):
    """one disjoint, contiguous block of host cores per rank (launch thread, autograd thread, HIP / RCCL helper threads of a
    rank stay off the other ranks' cores).  N = 1: nothing to separate, unless WAVLM_PIN_CORES=lo-hi asks for a block."""
    if not hasattr(os, "sched_setaffinity"):
        return None
    spec = os.environ.get("WAVLM_PIN_CORES")
    try:
        avail = sorted(os.sched_getaffinity(0))
        if spec:
            lo, hi = (int(v) for v in spec.split("-"))
            cores = [c for c in avail if lo <= c <= hi]
        elif local_world > 1:
            per = max(1, len(avail) // local_world)
            cores = avail[local_rank * per:(local_rank + 1) * per]
        else:
            return None
        if cores:
            os.sched_setaffinity(0, cores)
            return "%d-%d" % (cores[0], cores[-1])
    except (OSError, ValueError):
        pass
    return None


def busy_and_enqueue(step, reps=5):
    """(gpu_busy_ms, host_enqueue_ms) of one step, medians over `reps`: the GPU is first parked on a spin kernel
    (torch.cuda._sleep) and two un-measured steps (so that the measured one sees the clocks of a steady stream of steps),
    the measured step is enqueued behind them -- the launch thread is never waiting for the GPU and the GPU never for the launch thread -- and
    two events around it give the time the GPU needs when nothing starves it; the host clock around the same call gives
    what the launch thread needs to enqueue it.  ms_per_step of the timed region within a few % of gpu_busy = the step is
    GPU-bound on this box; ms_per_step ~ host_enqueue = launch-bound."""
    # calibrate the spin kernel: cycles per ms on this part
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); torch.cuda._sleep(20_000_000); e1.record()
    torch.cuda.synchronize()
    per_ms = 20_000_000 / max(e0.elapsed_time(e1), 1e-3)
    busy, host = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        # a short spin gives the host its head start; the FIRST step behind it is the one whose enqueue time is taken (the
        # runtime's queues are empty: nothing but the launch thread's own work is in that number -- three steps deep the HIP
        # runtime drains its command batches and the launch thread waits for the GPU); then one more unmeasured step -- the
        # part is power-limited, a step that follows an idle (spinning) GPU runs ~4 % faster than one in a steady stream of
        # steps (measured 33.1 against 34.5 ms), the measured step must see the clocks of the timed region -- and the step
        # whose GPU time is taken between two events
        torch.cuda._sleep(int(per_ms * 20))
        t0 = time.perf_counter()
        step()
        t1 = time.perf_counter()
        step()
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        busy.append(e0.elapsed_time(e1))
        host.append((t1 - t0) * 1e3)
    busy.sort(); host.sort()
    return busy[len(busy) // 2], host[len(host) // 2]


def run_alt_pass(args, rank, world, dev, native=False):
    """every rank starts one child `bench.py` (same rank, same GPU, new rendezvous port hosted by rank 0's child) with
    NCCL_MAX_NCHANNELS removed and WAVLM_DP_RESERVED_CUS=0 -- or, native=True, with the DEFAULT channel cap / reservation and
    the library's own RCCL reducer as the transport (WAVLM_DP_NATIVE=1: the other untested default) --, waits for it, and rank 0
    returns the child's headline numbers.  Failures (time-out, no line) are reported, never raised: the primary measurement is
    already taken."""
    import subprocess
    port = [_free_port() if rank == 0 else 0]
    dist.broadcast_object_list(port, src=0)
    env = dict(os.environ)
    for k in ("NCCL_MAX_NCHANNELS", "TORCHELASTIC_USE_AGENT_STORE"):
        env.pop(k, None)
    env.update(MASTER_PORT=str(port[0]), MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"))
    if native:
        env.update(WAVLM_DP_NATIVE="1")
        if os.environ.get("NCCL_MAX_NCHANNELS"):
            env["NCCL_MAX_NCHANNELS"] = os.environ["NCCL_MAX_NCHANNELS"]
    else:
        env.update(WAVLM_DP_RESERVED_CUS="0")
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(args.gpus), "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--batch", str(args.batch), "--config", args.config, "--full", "--dp-alt-pass", "never", "--no-cpu-baseline", "--no-roofline"]
    torch.cuda.synchronize()
    res = {"settings": {"WAVLM_DP_NATIVE": 1, "NCCL_MAX_NCHANNELS": env.get("NCCL_MAX_NCHANNELS")} if native
           else {"NCCL_MAX_NCHANNELS": None, "WAVLM_DP_RESERVED_CUS": 0}}
    try:
        # (a child is an ordinary short run: ~1 min with start-up; the bound keeps a stuck rendezvous from holding the primary line back)
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), None)
        if rank == 0:
            if line is None:
                res["error"] = "no result line (rc %d): %s" % (r.returncode, r.stderr[-300:])
            else:
                d = json.loads(line)
                dp2 = d.get("data_parallel") or {}
                res.update(value=d["value"], ms_per_step=d["ms_per_step"], comm_wait_ms_per_rank=dp2.get("comm_wait_ms_per_rank"),
                           exposed_ms_last_bucket_rank0=dp2.get("exposed_ms_last_bucket_rank0"),
                           allreduce_bus_gb_s_rank0=dp2.get("allreduce_bus_gb_s_rank0"), buckets_rank0=dp2.get("buckets_rank0"))
    except Exception as e:   # noqa: BLE001 -- a diagnostic leg must not take the measurement down
        res["error"] = "%s: %s" % (type(e).__name__, e)
    dist.barrier()
    return res


DUMP_BYTES = 64 * 2 ** 20    # --dump-outputs: hard limit of what one run writes
DUMP_SAMPLE_BYTES = 32 * 2 ** 20   # ... and what the samples of the large tensors are sized for


def training_state(opt, dev):
    """what a training step reads besides the batch: the optimizer arenas (bf16 parameters, fp32 master, moments), the step
    count, and the host / device random streams (masks, mixing plans, dropout seeds, instance sampling)"""
    from unispeech_amd import functional as WF
    return {"arenas": [t.clone() for t in (opt.flat_param, opt.master, opt.exp_avg, opt.exp_avg_sq)], "step": opt.step_count,
            "np": np.random.get_state(), "torch": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(dev),
            "seed_ctr": WF._SEED_CTR[0]}


def restore_training_state(opt, dev, st):
    from unispeech_amd import functional as WF
    for dst, src in zip((opt.flat_param, opt.master, opt.exp_avg, opt.exp_avg_sq), st["arenas"]):
        dst.copy_(src)
    opt.step_count = st["step"]
    opt._params_written()
    np.random.set_state(st["np"])
    torch.set_rng_state(st["torch"])
    torch.cuda.set_rng_state(st["cuda"], dev)
    WF._SEED_CTR[0] = st["seed_ctr"]


def _sample_index(name, numel, k):
    """k sorted flat indices of a tensor of numel elements, seeded by its name only (identical from run to run and build to build)"""
    if k >= numel:
        return None
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return np.sort(rng.choice(numel, size=k, replace=False))


def _sampled(name, t, k):
    flat = t.detach().reshape(-1)
    idx = _sample_index(name, flat.numel(), k)
    if idx is not None:
        flat = flat[torch.from_numpy(idx).to(flat.device)]
    return flat.float().cpu().numpy()


def step_outputs(result, sample_size, model, extract):
    """{name: float32 / float64 array} of what the last step handed its caller: the features of an extract call, or the loss,
    the sample size and every parameter's gradient and updated value of a training step.  Larger tensors are represented by a
    fixed sample of their elements (_sample_index) sized to DUMP_SAMPLE_BYTES in all."""
    if extract:
        return {"features": _sampled("features", result, DUMP_SAMPLE_BYTES // 4)}
    out = {"loss": np.asarray(float(result.item()), dtype=np.float64),
           "sample_size": np.asarray(float(sample_size), dtype=np.float64)}
    named = [(n, p) for n, p in model.named_parameters() if p.grad is not None]
    # per-tensor cap: the largest power of two whose gradient + parameter samples fit the budget
    cap = 2 ** 24
    while cap > 1 and 2 * 4 * sum(min(p.numel(), cap) for _, p in named) > DUMP_SAMPLE_BYTES:
        cap //= 2
    for n, p in named:
        out["grad." + n] = _sampled(n, p.grad, cap)
        out["param." + n] = _sampled(n, p, cap)
    return out


def write_outputs(path, arrays):
    os.makedirs(path, exist_ok=True)
    total = 0
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        total += a.nbytes
        np.save(os.path.join(path, name + ".npy"), a)
    assert total <= DUMP_BYTES, total


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=BATCH_PER_GPU)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="base",
                    help="base = BASELINE.json configs[1] (the headline); large = WavLM-Large, 20 s utterances; "
                         "sat_large = UniSpeech-SAT Large with utterance mixing + contrastive head; extract = eval "
                         "extract_features per call on the configs[1] batch")
    ap.add_argument("--full", action="store_true",
                    help="report / run every leg besides the headline (ms_per_step_unsettled, gpu_busy / host_enqueue, "
                         "roofline, cpu_baseline, secondary, the data_parallel block and its alternative passes), all outside "
                         "the timed steps; without it a run sets up, warms up, settles, times the steps, dumps if asked and "
                         "prints the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the cpu_baseline leg")
    ap.add_argument("--no-roofline", action="store_true", help="--full without the roofline leg")
    ap.add_argument("--no-settle", action="store_true", help="skip the untimed settling steps after the warm-up")
    ap.add_argument("--no-busy", action="store_true", help="--full without the gpu_busy / host_enqueue leg")
    ap.add_argument("--no-secondary", action="store_true",
                    help="--full without the `secondary` leg (N = 1, config base: 5 steps each of --config large and --config "
                         "extract in fresh processes on the same GPU after the headline is taken)")
    ap.add_argument("--live-traffic", action="store_true",
                    help="with --full: collect roofline.traffic live (two rocprofv3 PMC passes of this command as subprocesses, ~1 min)")
    ap.add_argument("--dp-alt-pass", choices=["auto", "always", "never"], default="auto",
                    help="N > 1, with --full: second measurement with NCCL_MAX_NCHANNELS unset and no reserved CUs (fresh processes "
                         "on the same GPUs); auto = when a rank waits > 1 ms for the gradient all-reduce after backward")
    ap.add_argument("--force-dp", action="store_true",
                    help="1 GPU: run the step through the data-parallel machinery of a rank (DataParallelWavLM over a one-rank gloo "
                         "group: bucketed reducer on its side stream, gradient listeners, reserved CUs, the sample-size all-reduce) -- "
                         "what the N > 1 path costs a rank before any byte crosses a link; with --full the line carries a "
                         "`data_parallel` block")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed to DIR/<name>.npy (float32 / float64, "
                         "at most 64 MB in all): training configs the loss, the sample size and, per parameter, a fixed seeded "
                         "sample of its gradient and of its updated value; extract a fixed seeded sample of the features.  The "
                         "timed steps then start from the state after the warm-up (the settling steps are undone), so that two "
                         "runs with the same arguments compute from identical inputs")
    ap.add_argument("--reserved-cus", type=int, default=-1,
                    help="1 GPU: shrink the persistent GEMM grids by this many CUs as the data-parallel reducer does "
                         "(WAVLM_DP_RESERVED_CUS) -- what the reservation alone costs a rank")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full and (args.live_traffic or args.dp_alt_pass == "always"):
        ap.error("--live-traffic and --dp-alt-pass always belong to legs that only --full runs")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: become the launcher (one rank per GPU, rendezvous on 127.0.0.1),
        # the counterpart of distributed_utils.call_main spawning the ranks (src/fairseq/distributed/utils.py:332-367)
        if os.environ.get("WAVLM_SHARED_GPU") != "1" and torch.cuda.device_count() < args.gpus:
            raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible" % (args.gpus, torch.cuda.device_count()))
        import subprocess
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d rank(s)" % (args.gpus, world))
    SECONDS = CONFIGS[args.config]["seconds"]
    # WAVLM_SHARED_GPU=1 + WAVLM_DIST_BACKEND=gloo: functional test of the N > 1 path on a single-GPU box (all ranks on
    # cuda:0, gradients reduced through gloo); the real thing is one rank per GPU over RCCL ("nccl")
    if os.environ.get("WAVLM_SHARED_GPU") == "1":
        local_rank = 0
    backend = os.environ.get("WAVLM_DIST_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    pinned = pin_rank_cores(int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("LOCAL_WORLD_SIZE", str(world))))
    force_dp = bool(args.force_dp) and world == 1
    if force_dp:
        # one rank of RCCL on this GPU (an all-reduce is an in-place copy kernel then), everything else as in a real N > 1
        # run: channel cap in the environment before the communicator exists, reducer forced on, CUs reserved
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        os.environ["WAVLM_DP_FORCE"] = "1"
        from unispeech_amd.dp import cap_rccl_channels
        cap_rccl_channels(2)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    dp = world > 1 or force_dp   # the step runs through the data-parallel wrapper
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RCCL gets as many channels (= workgroups = CUs) as the persistent GEMM grids leave free (unispeech_amd/dp.py)
        from unispeech_amd.dp import cap_rccl_channels
        cap_rccl_channels(world)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from unispeech_amd import functional as WF
    from unispeech_amd import hostenv, ops
    # the launch thread must not share a throttled cgroup with a 256-thread OpenMP pool (unispeech_amd/hostenv.py)
    host_threads = hostenv.cap_threads(4)
    if args.reserved_cus >= 0 and world == 1:
        ops.set_reserved_cus(args.reserved_cus)
    from unispeech_amd.dp import DataParallelWavLM
    from unispeech_amd.optim import FusedAdam
    from unispeech_amd.pretrain import WavLMCriterion, WavLMPretrainModel

    extract = bool(CONFIGS[args.config].get("extract"))
    torch.manual_seed(0)
    if extract:
        from unispeech_amd.wavlm import WavLM
        model = WavLM(extract_cfg()).to(dev).to(torch.bfloat16).eval()
        opt = net = None
        # a frozen feature extractor: the caller states that nothing writes the parameters between calls, so the tensors derived
        # from them alone (packed q|k|v, conv / pos_conv GEMM images) are kept (opt-in since round 6: functional.set_eval_cache)
        WF.set_eval_cache(True)
    else:
        cfg = base_cfg(True, args.config)
        model = WavLMPretrainModel(cfg, None, [range(V)]).to(dev).to(torch.bfloat16).train()
        opt = FusedAdam(model.parameters(), lr=5e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.01, clip_norm=10.0, model=model)
        model.instance_sampling = "device"   # UniSpeech-SAT head: draw the instance indices on the GPU (no host work per step)
        net = DataParallelWavLM(model, opt, bucket_bytes=int(float(os.environ.get("WAVLM_DP_BUCKET_MIB", "32")) * 2 ** 20)) \
            if dp else model
    sat = bool(CONFIGS[args.config].get("sat"))
    crit = WavLMCriterion(None, 1.0, 0.0, loss_weights=[10.0, 10.0, 0.0] if sat else [10.0], defer_logging=True)

    B, T = args.batch, int(SECONDS * SR)
    g = torch.Generator().manual_seed(1234 + rank)
    wav = torch.randn(B, T, generator=g).to(dev).to(torch.bfloat16)
    pm_cpu = torch.zeros(B, T, dtype=torch.bool)
    sample = {"id": torch.arange(B),
              "net_input": {"source": wav, "padding_mask": pm_cpu.to(dev), "padding_mask_cpu": pm_cpu},
              "target_list": [torch.randint(4, V, (B, int(50 * SECONDS)), generator=g).to(dev)]}
    np.random.seed(1337 + rank)
    torch.manual_seed(1337)
    mixer = None
    if sat:
        # utterance mixing of the collated batch, as UtteranceMixingDataset.collater does it (host draws, device arithmetic)
        from unispeech_amd.data import UtteranceMixingCollater
        mixer = UtteranceMixingCollater(mixing_prob=0.5, mixing_num=1, normalize=True, device=dev)
        raw = torch.randn(B, T, generator=g).to(dev)          # fp32 un-mixed batch, resident before the timed region
        zero_rows = [False] * B

    def step():
        if extract:   # one call of the public API: waveform [B, T] -> last-layer features [B, T', D] (no mask, eval)
            with torch.no_grad():
                feats, _ = model.extract_features(wav)
            return feats
        opt.zero_grad()
        if mixer is not None:
            ops_np, begin_np, _ = mixer.draw_mixing_plan(B, T, zero_rows)
            sample["net_input"]["source"] = ops.mix_utterances(raw, WF.h2d(ops_np.reshape(-1), dev), ops_np.shape[0],
                                                                WF.h2d(begin_np, dev), None, True, torch.bfloat16)
        loss, ss, _ = crit(net, sample)
        last_ss[0] = ss
        loss.backward()
        if dp:
            if comm_ev is not None:
                comm_ev[0].record()      # end of backward on the compute stream
            net.all_reduce_grads()   # AVERAGE over ranks (the wrapper folds 1/world into the optimizer's deferred factor)
            if comm_ev is not None:
                comm_ev[1].record()      # the compute stream has waited for every bucket's all-reduce
            # pinned + asynchronous: torch.tensor(..., device=dev) is a blocking H2D copy, i.e. a stream synchronisation
            # that would cost the launch thread its run-ahead in every data-parallel step
            sst = WF.h2d(torch.tensor([float(ss)], dtype=torch.float32), dev)
            dist.all_reduce(sst)
            # trainer.py:796-801: multiply_grads(world / sample_size summed over ranks)
            opt.step(grad_mult=float(world), grad_mult_dev=sst.reciprocal())
        else:
            opt.step(grad_mult=1.0 / max(ss, 1))
        return loss

    comm_ev = None   # set for the communication-wait leg after the timed region
    last_ss = [None]  # sample size of the latest training step (--dump-outputs)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    # --dump-outputs: the untimed steps between the warm-up and the timed region are not a fixed number (settling), so the
    # training state after the warm-up is kept and put back in front of the timed steps
    after_warmup = training_state(opt, dev) if (args.dump_outputs and opt is not None) else None
    # Settling: the first heavy process on a fresh box (or right after another GPU job) has been measured 10-20 % slow for
    # its first seconds (clocks / power state; 41.4 ms then 34.4 ms for two back-to-back runs of this script).  After the W
    # warm-up steps, up to 15 more UNTIMED steps run until two consecutive steps agree within 2 % (N > 1: five steps on every rank, the
    # steps are collective); the count is reported as `settle_steps`.  The timed region below is unchanged: exactly K steps between two fences.
    settle = 0
    settle_host_ms = None
    unsettled_ms = None
    if not args.no_settle and world == 1:
        # K steps right after the warm-up, in front of the settling loop.  Every run takes them: they are part of what
        # precedes the timed region (without them the timed steps measured ~0.35 % slower, 33.65 against 33.53 ms, same
        # box, alternating runs).  --full also reports their time as `ms_per_step_unsettled`, the r02 methodology (no
        # settling steps), so that rounds stay comparable like for like
        torch.cuda.synchronize()
        tu = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        if args.full:
            unsettled_ms = (time.perf_counter() - tu) / args.steps * 1e3
    if not args.no_settle and world > 1:
        for _ in range(5):  # a fixed count: every rank must run the same number of (collective) steps
            step()
            settle += 1
    elif not args.no_settle:
        # two things settle here, both untimed: the GPU's clocks (two consecutive steps within 2 %) and the HOST -- on a
        # freshly acquired box the launch thread has been measured 5-8 x slower for its first tens of seconds (enqueue 26-58
        # ms per step against 6; page cache, frequency governor, the box's own start-up work), which makes the step
        # launch-bound until it passes.  While a step's enqueue time exceeds half of its wall time the loop keeps going, for
        # at most 30 s; the count is reported as `settle_steps`, the last enqueue time as `settle_host_ms`.
        prev, t_settle0 = None, time.perf_counter()
        while True:
            torch.cuda.synchronize()
            ts = time.perf_counter()
            step()
            th = time.perf_counter() - ts
            torch.cuda.synchronize()
            cur_t = time.perf_counter() - ts
            settle += 1
            settle_host_ms = th * 1e3
            host_bound = th > 0.5 * cur_t
            stable = prev is not None and abs(cur_t - prev) <= 0.02 * prev
            prev = cur_t
            if host_bound:
                if time.perf_counter() - t_settle0 > 30.0:
                    break
                continue
            if stable or settle >= 15:
                break
    if after_warmup is not None:
        restore_training_state(opt, dev, after_warmup)
        after_warmup = None
    # the model, optimizer arenas and cached workspaces are long-lived: move them out of the cyclic collector's young
    # generations so that a full collection cannot stall the launch thread for milliseconds mid-step (a training loop
    # would do the same once after its first step)
    import gc
    gc.collect()
    gc.freeze()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    fence()
    dt = time.perf_counter() - t0
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = tmax.item()
    final_loss = float(loss.float().abs().mean().item()) if extract else float(loss.item())
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, step_outputs(loss, last_ss[0], model, extract))
    # second clock on the same build, outside the timed region: what the GPU needs for a step when the launch thread is not
    # in its way, and what the launch thread needs to enqueue one (see busy_and_enqueue)
    gpu_busy_ms, host_enq_ms = busy_and_enqueue(step) if (args.full and world == 1 and not args.no_busy) else (None, None)
    dp_info = None
    if dp:
        # what identifies the run as N ranks on N distinct devices over RCCL (no step: one collective after the timed region)
        props = torch.cuda.get_device_properties(dev)
        ident = "%s|%s" % (getattr(props, "uuid", None), getattr(props, "pci_bus_id", local_rank))
        gathered = [None] * world
        dist.all_gather_object(gathered, {"rank": rank, "device": ident, "pinned": pinned})
        gathered.sort(key=lambda g_: g_["rank"])
        try:
            rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            rccl = None
        dp_info = {"ranks_seen": len(gathered), "distinct_devices": len({g_["device"] for g_ in gathered}),
                   "backend": backend, "rccl_version": rccl,
                   # "torch": torch.distributed collectives on a side stream; "native": the library's own RCCL reducer
                   # (wavlm_dp_*, WAVLM_DP_NATIVE=1; no per-bucket events: buckets_rank0 is null then)
                   "transport": "native" if net.reducer.transport is not None else "torch",
                   "host_cores_per_rank": [g_["pinned"] for g_ in gathered]}
    if dp and args.full:
        # evidence for the overlap of the gradient all-reduce with backward, from the driver's own run: per rank, the time
        # the compute stream waits between the end of backward and the completion of the last bucket (0 = fully hidden)
        waits = []
        comm_ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        for _ in range(3):
            step()
            torch.cuda.synchronize()
            waits.append(comm_ev[0].elapsed_time(comm_ev[1]))
        # per-bucket picture of one step (diagnostic steps, outside the timed region): when each bucket's all-reduce was
        # launched relative to the end of backward, how long it ran, its bus bandwidth, and what the LAST bucket (extractor +
        # first blocks: nothing left to hide behind) leaves exposed
        red = net.reducer
        bucket_rows, exposed_last = None, None
        if red.comm_stream is not None:
            red.record_timing = True
            per = {}
            for _ in range(3):
                red.timing = []
                step()
                torch.cuda.synchronize()
                for (bi, nbytes, ev_l, e0, e1) in red.timing:
                    per.setdefault(bi, []).append((nbytes, ev_l.elapsed_time(comm_ev[0]), e0.elapsed_time(e1), comm_ev[0].elapsed_time(e1)))
            red.record_timing = False
            busf = 2.0 * (world - 1) / world        # ring all-reduce: bytes on the busiest link per byte reduced
            bucket_rows = []
            for bi in sorted(per):
                v = sorted(per[bi], key=lambda t: t[2])[len(per[bi]) // 2]
                bucket_rows.append({"bucket": bi, "mib": round(v[0] / 2 ** 20, 1), "launched_ms_before_backward_end": round(v[1], 3),
                                    "allreduce_ms": round(v[2], 3), "bus_gb_s": round(v[0] * busf / max(v[2], 1e-6) / 1e6, 1),
                                    "ends_ms_after_backward_end": round(v[3], 3)})
            if bucket_rows:
                exposed_last = max(0.0, bucket_rows[-1]["ends_ms_after_backward_end"])
        comm_ev = None
        waits.sort()
        waits_all = [None] * world
        dist.all_gather_object(waits_all, round(waits[1], 3))
        dp_info.update({"buckets": len(red.buckets),
                        "bucket_mib": round(net._bucket_bytes / 2 ** 20, 1), "reserved_cus": ops.get_reserved_cus(),
                        "grad_arena_mib": round(opt.flat_grad.numel() * opt.flat_grad.element_size() / 2 ** 20, 1),
                        "grad_sum_dtype": str(opt.flat_grad.dtype).replace("torch.", ""),
                        "rccl_max_nchannels": os.environ.get("NCCL_MAX_NCHANNELS"),
                        # (rank 0's view, median of three diagnostic steps; bus_gb_s = bytes x 2 (N - 1) / N / time: compare with
                        # one xGMI link, ~153 GB/s -- the cap NCCL_MAX_NCHANNELS = reserved CUs is a hypothesis)
                        "buckets_rank0": bucket_rows, "exposed_ms_last_bucket_rank0": exposed_last,
                        "allreduce_bus_gb_s_rank0": None if not bucket_rows else round(
                            sum(r_["mib"] for r_ in bucket_rows) * 2 ** 20 * (2.0 * (world - 1) / world)
                            / max(sum(r_["allreduce_ms"] for r_ in bucket_rows), 1e-6) / 1e6, 1),
                        "comm_wait_ms_per_rank": waits_all})

    # N > 1, self-diagnosis on the first real node (nobody could tune this beforehand: RCCL has never executed in the build
    # environment): when a rank waits noticeably for the all-reduce after backward -- or on request -- the same measurement
    # runs once more in FRESH processes on the same GPUs with the two untested choices reverted: NCCL_MAX_NCHANNELS unset
    # (RCCL picks its own channel count) and no CUs reserved (full persistent grids).  Fresh processes, because RCCL reads
    # its environment once per process.  Both results go into `data_parallel`; the headline stays the default configuration's.
    alt = None
    if args.full and world > 1 and dp_info is not None and args.dp_alt_pass != "never":
        worst_wait = max(dp_info["comm_wait_ms_per_rank"])
        if args.dp_alt_pass == "always" or worst_wait > 1.0:
            alt = run_alt_pass(args, rank, world, dev)
            # ... and the transport nobody has run on more than one rank: the reducer below Python (wavlm_dp_*), same channel
            # cap and reservation as the headline.  It stays opt-in until a node shows it ahead
            # (RCCL only: two ranks of the functional gloo / shared-GPU mode cannot form an RCCL communicator on one device)
            alt_native = (run_alt_pass(args, rank, world, dev, native=True)
                          if (dp_info["transport"] == "torch" and backend == "nccl" and os.environ.get("WAVLM_SHARED_GPU") != "1") else None)
            if rank == 0:
                dp_info["alt_pass"] = alt
                dp_info["alt_pass_native"] = alt_native

    roof = None
    if args.full and not args.no_roofline:
        # Three single-step passes, the one with the smallest GEMM time is reported.  The events bracket each launch ON THE
        # STREAM; with the events' own host cost the launch thread runs level with the GPU, so one of the HIP runtime's
        # periodic launch stalls (tens of ms every ~2000 launches on these boxes) lands between an event and its kernel
        # and is booked as kernel time (observed once: 40 ms of "GEMM time" in a 36 ms step).  A stall can only inflate.
        best, passes = None, []
        for _ in range(3):
            ops.prof_enable(True)
            step()
            got = (ops.prof_collect(1), ops.prof_collect_bytes(1), kernel_rooflines(ops, 1))
            ops.prof_enable(False)
            if got[0][1] > 0:
                passes.append(got[0][1])
            if got[0][1] > 0 and (best is None or got[0][1] < best[0][1]):
                best = got
        (n_l, ms, fl), alg_bytes, kern = best if best is not None else ((0, 0.0, 0.0), 0.0, [])
        if ms > 0:
            ach = fl / (ms * 1e-3) / 1e12
            # HBM bytes per GEMM launch: counters cannot be read from inside the run.  --live-traffic collects them NOW with
            # two rocprofv3 PMC passes of this same command in subprocesses (FETCH_SIZE x 2 on gfx950, WRITE_SIZE, each with
            # --kernel-trace only, as /opt/skills/guides/MI355X_MICROARCH.md prescribes); the default reads the passes
            # committed with the latest round's build (tools/gpu_pmc.sh -> profiles/rNN/gemm_hbm_traffic_<config>.json) and says so
            traffic, traffic_src, traffic_launches = None, None, None
            if args.live_traffic and world == 1:
                traffic, traffic_src, traffic_launches = live_gemm_traffic(args)
            if traffic is None and args.batch == BATCH_PER_GPU:
                # the passes committed with the round's build, per config (tools/gpu_pmc.sh -> gemm_hbm_traffic_<config>.json)
                import glob
                cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]", "gemm_hbm_traffic_%s.json" % args.config)))
                tj = cands[-1] if cands else ""
                if os.path.exists(tj):
                    try:
                        tjd = json.load(open(tj))
                        traffic = round(tjd["gemm_hbm_bytes_per_launch"])
                        traffic_launches = tjd["gemm_launches_per_step"]
                        traffic_src = "%s (committed rocprofv3 PMC passes of this command, not this run; `bench.py " \
                                      "--live-traffic` collects them live)" % os.path.relpath(tj, ROOT)
                    except Exception:
                        traffic = None
            roof = {"bound": "mfma",
                    "kernel": "bf16 MFMA GEMM family (gemm_pp_kernel / gemm_w4_kernel 256x256, gemm_pp3_kernel 192x384, gemm_bf16_kernel "
                              "128-wide): every dense contraction of the step that goes through wavlm_gemm (all but the fused "
                              "attention and the direct pos_conv kernels)",
                    "achieved": round(ach, 1), "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(ach / BF16_MFMA_PEAK_TFLOPS, 4), "traffic": traffic,
                    "traffic_unit": "HBM bytes per launch (avg over the step's GEMM launches, PMC)",
                    "power_note": "measured, not live (profiles/r04/power_probe.txt): every GEMM of the step runs the socket at its "
                                  "1400 W limit (clock traded against active CUs); the vendor library's 8192^3 reaches 1402 TFLOP/s "
                                  "= 0.56 of `peak` inside that envelope",
                    "traffic_source": traffic_src,
                    # the counters and the library's own launch record must describe the same set of launches (VERDICT r4:
                    # a name filter had dropped the step's largest GEMM kernel from the counters' side)
                    "traffic_launches_per_step": traffic_launches,
                    "traffic_launches_match": None if traffic_launches is None else bool(abs(traffic_launches - n_l) < 0.5),
                    "algorithmic_bytes_per_launch": round(alg_bytes / max(n_l, 1)),
                    "launches_per_step": n_l, "gemm_ms_per_step": round(ms, 3),
                    # (the best of three passes is the optimistic one -- the median and its frac are here too)
                    "gemm_ms_per_step_median_of_3": round(sorted(passes)[len(passes) // 2], 3) if passes else None,
                    "frac_median_of_3": round(fl / (sorted(passes)[len(passes) // 2] * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4) if passes else None,
                    "gemm_algorithmic_tflop_per_step": round(fl / 1e12, 3),
                    "avg_launch_us": round(ms / max(n_l, 1) * 1e3, 2),
                    "kernels": kern}
    fence()

    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        value = world * B * SECONDS * args.steps / dt
        c = CONFIGS[args.config]
        Tp = T
        for k_, s_ in [(10, 5)] + [(3, 2)] * 4 + [(2, 2)] * 2:
            Tp = (Tp - k_) // s_ + 1
        out = {
            "metric": "audio-seconds/sec %s, %s %ds@16kHz" % ("extract_features" if extract else "pretraining",
                                                            c["name"].split(" (")[0], int(SECONDS)),
            "value": round(value, 1),
            "unit": "audio-s/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "gpu_busy_ms_per_step": None if gpu_busy_ms is None else round(gpu_busy_ms, 2),
            "host_enqueue_ms_per_step": None if host_enq_ms is None else round(host_enq_ms, 2),
            "host_cores_pinned": pinned, "host_threads": host_threads, "host_cpu_quota": hostenv.cpu_quota(),
            "reserved_cus": ops.get_reserved_cus(),
            "settle_steps": settle,
            "settle_host_ms": None if settle_host_ms is None else round(settle_host_ms, 2),
            "ms_per_step_unsettled": None if unsettled_ms is None else round(unsettled_ms, 2), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "synthetic",
            "config": {"workload": ("%s extract_features (eval forward, no mask), bf16, batch=%dx%ds per GPU (%s%s)"
                                    if extract else
                                    "%s pretrain fwd+bwd+grad-reduce+fused-Adam, bf16, batch=%dx%ds per GPU, masked-pred loss (%s%s)")
                                   % (c["name"], B, int(SECONDS), c["baseline"], "" if world == 1 else ", dp%d" % world),
                       "global_batch": world * B, "seconds_per_utt": SECONDS, "frames_per_utt": Tp,
                       "parallelism": "dp%d" % world, "dropout": 0.1, "attention_dropout": 0.1, "layerdrop": 0.0,
                       "mask_prob": 0.8, "optimizer": "fused Adam, fp32 master, clip 10"},
            "final_loss": final_loss,
            "model_tflops": round(algorithmic_flops_per_step(B, T, args.config) / (1.0 if not extract else 3.0)
                                  / (ms_per_step * 1e-3) / 1e12, 1),
        }
        if extract:
            out["config"].update(dropout=0.0, attention_dropout=0.0, optimizer=None, mask_prob=0.0, eval_cache=True)
            out.pop("final_loss")
            out["mean_abs_feature"] = final_loss
        if dp_info is not None:
            # what identifies the run as N ranks on N devices over RCCL, at the top level where a SCALE parser looks first
            out.update(ranks_seen=dp_info["ranks_seen"], distinct_devices=dp_info["distinct_devices"],
                       rccl_version=dp_info["rccl_version"], dist_backend=dp_info["backend"], dp_transport=dp_info["transport"])
            a_ = dp_info.get("alt_pass")
            if a_ and a_.get("value"):
                dp_info["alt_pass_faster_than_default"] = bool(a_["value"] > 1.01 * value)
            n_ = dp_info.get("alt_pass_native")
            if n_ and n_.get("value"):
                dp_info["alt_pass_native_faster_than_default"] = bool(n_["value"] > 1.01 * value)
            if args.full:
                out["data_parallel"] = dp_info
        if roof is not None:
            out["roofline"] = roof
        if args.full and world == 1 and not args.no_cpu_baseline and args.config == "base":
            out["cpu_baseline"] = cpu_baseline()
        if args.full and world == 1 and not args.no_cpu_baseline and extract:
            out["cpu_baseline"] = cpu_baseline_extract()
        if (args.full and world == 1 and args.config == "base" and args.batch == BATCH_PER_GPU and not args.no_secondary
                and args.reserved_cus < 0):
            # two more of the five BASELINE configs in the same line: the headline is complete at this point (nothing below
            # touches its timed region); the model and its arenas are released and the other configs run as ordinary short
            # bench.py runs on the same GPU
            del sample, wav, crit, net, opt, model
            gc.collect()
            torch.cuda.empty_cache()
            out["secondary"] = secondary_lines()
        print(json.dumps(out), flush=True)
    if world > 1 or force_dp:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
