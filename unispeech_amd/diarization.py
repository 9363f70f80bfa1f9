"""Speaker diarization on the device: EEND with vector clustering over the upstream's layer states (csrc/diar.hip, ABI 24).

The inference path of the reference's downstreams/speaker_diarization: `models/models.py` (`TransformerDiarization`,
`feature_selection="hidden_states"`), `models/transformer.py` (the six-layer encoder) and the host stage of `diarization.py`
(chunking, silence / cannot-link lists, constrained average-linkage clustering, merge, stitching, median filter, RTTM).
  * `TransformerDiarization` -- parameter and buffer names equal the reference's, so a released checkpoint loads as in
    diarization.py:271-275 (`load_state_dict(fix_state_dict(ckpt["model"]), strict=False)`); the upstream's keys sit under
    `feature_extract.model.*`.
  * `hidden_states(wavs)` -- the L + 1 states of equal-length 16 kHz chunks, one upstream call; `forward_states(states,
    n_frames)` -- logits and per-frame speaker vectors; `estimate_states(states, n_frames)` -- activities and the weighted,
    normalised speaker vectors; `batch_estimate(wavs)` -- both steps.  All chunks of a recording have one length (the last
    one is shifted back), so a recording is ONE batch through the upstream and one through the head.
  * `chunk_recording`, `get_cl_sil`, `clustering`, `merge_acti_clslab`, `stitching`, `cluster`, `make_rttm`, `diarize` -- the
    host stage, numpy only.  `python -m unispeech_amd.diarization UPSTREAM.pt HEAD.pt CONFIG audio.wav`.
  * `predict` / `diarize` with `input_rate = model.sr` take the recording at the config's rate (8 kHz in the released config):
    chunks are cut at that rate and resampled to 16 kHz in one launch (unispeech_amd/resample.py), as the reference does.
Inference only (eval mode, no dropout, no gradients).  No CPU path and no eager fall-back for the kernels: every tensor-sized
step of the head is a libwavlm_hip.so entry point.  What torch does here is parameter-sized: the softmax of feature_weight
and the concatenated q|k|v and read-out weights (none of it under functional.frozen_parameters()).
"""
import itertools
import types

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import functional as F
from . import ops
from . import resample as _resample
from .speaker import Upstream, UpstreamStates, frame_count

__all__ = ["TransformerDiarization", "fix_state_dict", "chunk_recording", "get_cl_sil", "clustering", "merge_acti_clslab",
           "stitching", "cluster", "make_rttm", "diarize", "predict", "recording_chunks", "interp_taps", "medfilt_rows", "infer_args", "frame_count"]

UNFUSED_ATTENTION_MAX_T = 1024   # csrc/attn.hip: the upstream's unfused attention (fp32, or heads not 64 wide)


def fix_state_dict(state_dict):
    """strip `module.` (DataParallel) then `net.` (models.py:73-83)"""
    out = type(state_dict)() if isinstance(state_dict, dict) else {}
    for k, v in state_dict.items():
        if k.startswith("module."):
            k = k[7:]
        if k.startswith("net."):
            k = k[4:]
        out[k] = v
    return out


def interp_taps(T_in, T_out):
    """F.interpolate(mode="linear", align_corners=False) from T_in to T_out frames as (i0, i1, f): out[j] = (1 - f[j]) *
    x[i0[j]] + f[j] * x[i1[j]].  fp32 arithmetic in the kernel's order (csrc/diar.hip)."""
    j = np.arange(T_out, dtype=np.float32)
    scale = np.float32(T_in) / np.float32(T_out)
    src = np.maximum(scale * (j + np.float32(0.5)) - np.float32(0.5), np.float32(0.0)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), T_in - 1)
    i1 = np.minimum(i0 + 1, T_in - 1)
    return i0, i1, (src - i0.astype(np.float32)).astype(np.float32)


# ------------------------------------------------------------------------------------------ parameter containers
# (the reference's module tree, transformer.py:39-147: names only -- none of these modules' forward is ever called)
class MultiHeadSelfAttention(nn.Module):
    def __init__(self, n_units, h):
        super().__init__()
        self.linearQ = nn.Linear(n_units, n_units)
        self.linearK = nn.Linear(n_units, n_units)
        self.linearV = nn.Linear(n_units, n_units)
        self.linearO = nn.Linear(n_units, n_units)
        self.d_k, self.h = n_units // h, h


class PositionwiseFeedForward(nn.Module):
    def __init__(self, n_units, d_units):
        super().__init__()
        self.linear1 = nn.Linear(n_units, d_units)
        self.linear2 = nn.Linear(d_units, n_units)


class TransformerEncoder(nn.Module):
    def __init__(self, idim, n_layers, n_units, e_units=2048, h=8):
        super().__init__()
        self.linear_in = nn.Linear(idim, n_units)
        self.n_layers = n_layers
        for i in range(n_layers):
            setattr(self, "lnorm1_%d" % i, nn.LayerNorm(n_units))
            setattr(self, "self_att_%d" % i, MultiHeadSelfAttention(n_units, h))
            setattr(self, "lnorm2_%d" % i, nn.LayerNorm(n_units))
            setattr(self, "ff_%d" % i, PositionwiseFeedForward(n_units, e_units))
        self.lnorm_out = nn.LayerNorm(n_units)


class TransformerDiarization(UpstreamStates, nn.Module):
    """models.py:86-250 with feat_type = an upstream model and feature_selection="hidden_states".

    feat_dim: width D of the states; upstream: a unispeech_amd.wavlm.WavLM (its keys appear under feature_extract.model.*)
    or None for the head alone, in which case num_states (L + 1) must be given.  feat_type is kept for the config's sake (the
    reference reads a checkpoint path from it); only 'fbank' / 'mfcc' are refused.  sr / frame_shift: the rate the config
    counts frames in -- the waveform entry points take 16 kHz mono, what the reference holds after its resampler."""

    def __init__(self, n_speakers, all_n_speakers, feat_dim, n_units, n_heads, n_layers, dropout_rate=0.1, spk_emb_dim=256,
                 sr=8000, frame_shift=256, frame_size=1024, context_size=0, subsampling=1, feat_type="upstream",
                 feature_selection="hidden_states", interpolate_mode="linear", update_extract=False, feature_grad_mult=1.0,
                 upstream=None, num_states=None):
        super().__init__()
        if feat_type in ("fbank", "mfcc"):
            raise NotImplementedError("feat_type=%r: the torchaudio fbank / mfcc front ends are not built; the head runs on "
                                      "an upstream model's hidden states" % feat_type)
        if update_extract:
            raise NotImplementedError("update_extract=True (fine-tuning the upstream through the head) is not built: "
                                      "inference only")
        if context_size != 0:
            raise NotImplementedError("context_size=%r: splicing neighbouring frames is not built (context_size=0 only)"
                                      % (context_size,))
        if interpolate_mode != "linear":
            raise NotImplementedError("interpolate_mode=%r: only 'linear' is built" % (interpolate_mode,))
        if feature_selection != "hidden_states":
            raise NotImplementedError("feature_selection=%r: only 'hidden_states' is built" % (feature_selection,))
        if n_units % n_heads or n_units // n_heads != 32:
            raise NotImplementedError("n_units=%d / n_heads=%d: the attention kernel is built for heads 32 wide"
                                      % (n_units, n_heads))
        if spk_emb_dim > 512:
            raise NotImplementedError("spk_emb_dim=%d: the read-out kernel holds at most 512" % spk_emb_dim)
        self.context_size, self.subsampling = context_size, int(subsampling)
        self.feat_type, self.feature_selection = feat_type, feature_selection
        self.sr, self.frame_shift, self.frame_size = sr, frame_shift, frame_size
        self.interpolate_mode, self.update_extract, self.feature_grad_mult = interpolate_mode, update_extract, feature_grad_mult
        self.feat_dim, self.n_units, self.n_heads, self.spk_emb_dim = int(feat_dim), n_units, n_heads, spk_emb_dim
        self.dropout_rate = dropout_rate
        if upstream is not None:
            self.feature_extract = Upstream(upstream)
            n = len(upstream.encoder.layers) + 1
            if num_states is not None and num_states != n:
                raise ValueError("num_states=%d but the upstream yields %d hidden states" % (num_states, n))
            if upstream.cfg.encoder_embed_dim != feat_dim:
                raise ValueError("feat_dim=%d but the upstream's states are %d wide" % (feat_dim, upstream.cfg.encoder_embed_dim))
            num_states = n
            for p in self.feature_extract.parameters():
                p.requires_grad = False
        elif num_states is None:
            raise ValueError("num_states is required without an upstream")
        self.feat_num = int(num_states)
        self.feature_weight = nn.Parameter(torch.zeros(self.feat_num))
        self.instance_norm = nn.InstanceNorm1d(feat_dim)
        self.enc = TransformerEncoder(feat_dim, n_layers, n_units, h=n_heads)
        self.linear = nn.Linear(n_units, n_speakers)
        for i in range(n_speakers):
            setattr(self, "linear%d" % i, nn.Linear(n_units, spk_emb_dim))
        self.n_speakers = n_speakers
        self.embed = nn.Embedding(all_n_speakers, spk_emb_dim)
        self.alpha = nn.Parameter(torch.rand(1)[0] + torch.Tensor([0.5])[0])
        self.beta = nn.Parameter(torch.rand(1)[0] + torch.Tensor([0.5])[0])

    # -- derived weight images ---------------------------------------------------------------------------------------
    def _head_tensors(self):
        up = "feature_extract."
        return [t for n, t in list(self.named_parameters()) + list(self.named_buffers()) if not n.startswith(up)]

    def _build_images(self):
        im = {"w": torch.softmax(self.feature_weight.float(), dim=-1).contiguous()}
        for i in range(self.enc.n_layers):
            a = getattr(self.enc, "self_att_%d" % i)
            im["qkv_w%d" % i] = torch.cat([a.linearQ.weight, a.linearK.weight, a.linearV.weight]).contiguous()
            im["qkv_b%d" % i] = torch.cat([a.linearQ.bias, a.linearK.bias, a.linearV.bias]).contiguous()
        outs = [self.linear] + [getattr(self, "linear%d" % s) for s in range(self.n_speakers)]
        im["out_w"] = torch.cat([m.weight for m in outs]).contiguous()
        im["out_b"] = torch.cat([m.bias for m in outs]).contiguous()
        return im

    def _images(self):
        """softmax of feature_weight, the q|k|v weights of every layer and the read-out weights (linear | linear0 ..)
        concatenated: derived from the parameters per call, or kept under functional.frozen_parameters()"""
        return F.eval_derived(self._head_tensors(), "diar_images", self._build_images, inference=True)

    def load_state_dict(self, *a, **k):
        F.invalidate_derived()
        return super().load_state_dict(*a, **k)

    # -- refusals ------------------------------------------------------------------------------------------------------
    def _inference_only(self):
        if self.training:
            raise NotImplementedError("forward in training mode (dropout, update_extract, the PIT loss) is not built: call "
                                      ".eval()")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("forward with gradients required is not built (inference only): run under "
                                      "torch.no_grad()")

    def get_loss(self, *a, **k):
        raise NotImplementedError("get_loss (training: the PIT loss batch_pit_loss_parallel and the speaker loss) is not built: "
                                  "inference only")

    batch_estimate_with_perm = spk_loss_parallel = get_loss

    # -- upstream ------------------------------------------------------------------------------------------------------
    def n_frames(self, n_samples16):
        """frames the head yields for a 16 kHz chunk of n_samples16 (get_feat, models.py:193-195, on the sr-rate length)"""
        n_sr = int(n_samples16 * self.sr / 16000)
        return int(int(n_sr / self.frame_shift) / self.subsampling)

    def hidden_states(self, wavs):
        """[B, n] or a list of equal-length 1-D 16 kHz mono waveforms -> L + 1 tensors [B, T', D].  The waveform is
        layer-normed first when the upstream's cfg.normalize is set (UpstreamExpert.forward)."""
        self._inference_only()
        if not hasattr(self, "feature_extract"):
            raise ValueError("this head was built without an upstream: use forward_states")
        m = self.feature_extract.model
        wavs = self._wav_list(wavs)
        if len({len(w) for w in wavs}) != 1:
            raise ValueError("chunks of one recording have one length (chunk_recording shifts the last one back); got %s"
                             % sorted({len(w) for w in wavs}))
        p0 = next(m.parameters())
        frames = frame_count(len(wavs[0]), getattr(m.cfg, "conv_feature_layers"))
        hd = m.cfg.encoder_embed_dim // m.cfg.encoder_attention_heads
        fused = F.USE_FUSED_ATTENTION and p0.dtype == torch.bfloat16 and hd == 64
        if frames > UNFUSED_ATTENTION_MAX_T and not fused:
            raise ValueError("a chunk of %d samples is %d upstream frames, but this upstream (%s, heads %d wide) runs the "
                             "unfused attention, which stops at %d frames; a bf16 upstream with heads 64 wide (Base / Large) "
                             "has no such limit, or use a smaller chunk_size"
                             % (len(wavs[0]), frames, str(p0.dtype).replace("torch.", ""), hd, UNFUSED_ATTENTION_MAX_T))
        with torch.no_grad():
            return self._states_of(torch.stack(self._prepared_wavs(wavs)))

    # -- head ----------------------------------------------------------------------------------------------------------
    def _check_states(self, states):
        self._inference_only()
        if isinstance(states, torch.Tensor):
            states = list(states.unbind(0))
        states = [s if s.stride(-1) == 1 and s.stride(1) >= s.shape[2] else s.contiguous() for s in states]
        if len(states) != self.feat_num:
            raise ValueError("%d states given, feature_weight holds %d" % (len(states), self.feat_num))
        s0 = states[0]
        dev = ops._dev(s0)
        pd = self.enc.linear_in.weight.dtype
        if s0.dim() != 3 or s0.shape[2] != self.feat_dim or any(s.shape != s0.shape or s.dtype != s0.dtype or s.device != dev
                                                                for s in states):
            raise ValueError("states must share one shape [B, T', %d], dtype and device" % self.feat_dim)
        if s0.dtype != pd:
            raise TypeError("states are %s but the head's parameters are %s" % (s0.dtype, pd))
        return states

    def _encode(self, states, n_frames, inter=None):
        """get_feat (models.py:210-225) + TransformerEncoder.forward (transformer.py:126-147) -> [B * T, n_units]"""
        im = self._images()
        enc = self.enc
        B = states[0].shape[0]
        T = int(n_frames)
        if T < 1:
            raise ValueError("n_frames=%r" % (n_frames,))
        U, H = self.n_units, self.n_heads
        dev, dtype = states[0].device, states[0].dtype
        new = lambda *shape: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
        feat = ops.diar_front(states, im["w"], T, self.subsampling, 1e-6, self.instance_norm.eps)
        if inter is not None:
            inter["feat"] = feat
        M, D = B * T, self.feat_dim

        def linear(x, w, b, K, N):
            y = new(M, N)
            ops.gemm(x, w, y, M, N, K, lda=K, ldb=K, ldc=N, bias=b)
            return y

        def ln(x, r, mod):
            return ops.layernorm_fwd(x, r, mod.weight, mod.bias, mod.eps, save=False)[0]

        x, r = linear(feat, enc.linear_in.weight, enc.linear_in.bias, D, U), None
        for i in range(enc.n_layers):
            att, ff = getattr(enc, "self_att_%d" % i), getattr(enc, "ff_%d" % i)
            # e = lnorm1(e): the residual of the layer before (e + ff(e)) is summed inside the LayerNorm
            e1 = ln(x, r, getattr(enc, "lnorm1_%d" % i))
            qkv = linear(e1, im["qkv_w%d" % i], im["qkv_b%d" % i], U, 3 * U)
            o = ops.attn_plain_fwd(qkv.view(B, T, 3 * U), H)
            s = linear(o.view(M, U), att.linearO.weight, att.linearO.bias, U, U)
            # e = lnorm2(e + s): the residual is the NORMALISED tensor (transformer.py:134-140)
            e2 = ln(e1, s, getattr(enc, "lnorm2_%d" % i))
            E = ff.linear1.out_features
            h = linear(e2, ff.linear1.weight, ff.linear1.bias, U, E)
            _lib.check(_lib.lib().wavlm_spk_rowact(ops.ptr(h), ops.dt(h), M * E, E, ops.ptr(h), ops.dt(h), M * E, E, 1, M, E, 0,
                                                   None, None, None, None, ops.stream()), "wavlm_spk_rowact")   # ReLU
            x, r = e2, linear(h, ff.linear2.weight, ff.linear2.bias, E, U)
        emb = ln(x, r, enc.lnorm_out)
        if inter is not None:
            inter["enc"] = emb
        S, Es = self.n_speakers, self.spk_emb_dim
        z = linear(emb, im["out_w"], im["out_b"], U, S + S * Es)
        return z.view(B, T, S + S * Es)

    def forward_states(self, states, n_frames, intermediates=None):
        """states: L + 1 tensors [B, T', D] (or one [L + 1, B, T', D]) in the head's dtype, channel-last, read in place;
        n_frames: frames per chunk at the head's rate.  Returns (ys [B, T, S] logits, spksvecs: S tensors [B, T, E]) as
        forward() of the reference (models.py:232-250).  intermediates (a dict, optional) receives `feat` and `enc`."""
        states = self._check_states(states)
        with torch.no_grad():
            z = self._encode(states, n_frames, intermediates)
        S, E = self.n_speakers, self.spk_emb_dim
        return z[..., :S], [z[..., S + s * E:S + (s + 1) * E] for s in range(S)]

    def estimate_states(self, states, n_frames):
        """-> (activities fp32 [B, T, S], vectors [B, S, E]): batch_estimate / estimate (models.py:271-281, 325-344)"""
        states = self._check_states(states)
        with torch.no_grad():
            z = self._encode(states, n_frames)
            return ops.diar_estimate(z, self.n_speakers, self.spk_emb_dim)

    def batch_estimate(self, wavs):
        """[B, n] 16 kHz mono chunks of one length -> (activities [B, T, S], vectors [B, S, E])"""
        wavs = self._wav_list(wavs)
        return self.estimate_states(self.hidden_states(wavs), self.n_frames(len(wavs[0])))

    forward = batch_estimate


# ------------------------------------------------------------------------------------------------------------ host stage
# Written from the behaviour of the reference's diarization.py (its function names and argument order are kept so that a
# caller of one finds the other); the recorded results in tests/golden/diarization.npz are the check.
def infer_args(num_speakers=3, sil_spk_th=0.05, ahc_dis_th=1.0, clink_dis=1.0e4, session="Anonymous", threshold=0.4,
               median=25, **extra):
    """the inference options of the reference's command line, with its defaults"""
    return types.SimpleNamespace(num_speakers=num_speakers, sil_spk_th=sil_spk_th, ahc_dis_th=ahc_dis_th, clink_dis=clink_dis,
                                 session=session, threshold=threshold, median=median, **extra)


def chunk_recording(audio_len, chunk_size, frame_shift, subsampling=1):
    """-> ([(start, end)] sample spans at the config's rate, [new frames per chunk]).  n_full whole chunks of chunk_size
    frames; a remainder becomes one more chunk of the SAME length that ends at audio_len (it starts inside its predecessor,
    or at 0 for a recording shorter than one chunk), of which only the remainder's whole frames are new."""
    hop = int(frame_shift * subsampling)
    size = chunk_size * hop
    n_full, tail = divmod(int(audio_len), size)
    spans = [(i * size, (i + 1) * size) for i in range(n_full)]
    new_frames = [chunk_size] * n_full
    if tail:
        spans.append((max(0, audio_len - size), audio_len))
        new_frames.append(tail // hop)
    return spans, new_frames


def get_cl_sil(args, acti, cls_num):
    """-> (cannot-link pairs, silent slots), both as indices chunk * n + slot in that order.  A slot is silent when its mean
    activity over the chunk is at most sil_spk_th; with a known cluster count below the slot count the weakest slot of every
    chunk is silent whatever its level.  Two active slots of one chunk that are cyclic neighbours (s, s + 1 mod n) cannot
    be one speaker."""
    n = args.num_speakers
    mean = np.stack([np.asarray(a).mean(axis=0) for a in acti]).astype(np.float64).reshape(len(acti), n)
    if cls_num is not None and n > cls_num:
        mean[np.arange(len(mean)), mean.argmin(axis=1)] = 0.0
    active = mean > args.sil_spk_th
    sil_lst = [int(i) for i in np.flatnonzero(~active.reshape(-1))]
    nxt = np.roll(active, -1, axis=1)
    cl_lst = [(c * n + s, c * n + (s + 1) % n) for c, s in zip(*np.nonzero(active & nxt))]
    return [(int(a), int(b)) for a, b in cl_lst], sil_lst


def average_linkage(dist, n_clusters=None, distance_threshold=None):
    """agglomerative clustering with average linkage on a precomputed distance matrix: merge the closest pair of clusters
    (mean of the pairwise distances) while that distance is below distance_threshold, or until n_clusters remain.  Labels are
    numbered by first appearance.  O(N^3): N is chunks x speakers."""
    dist = np.asarray(dist, dtype=np.float64)
    N = len(dist)
    members = [[i] for i in range(N)]
    while len(members) > (n_clusters if n_clusters is not None else 1):
        best, pair = None, None
        for a in range(len(members)):
            for b in range(a + 1, len(members)):
                d = dist[np.ix_(members[a], members[b])].mean()
                if best is None or d < best:
                    best, pair = d, (a, b)
        if n_clusters is None and best >= distance_threshold:
            break
        a, b = pair
        members[a] = members[a] + members[b]
        del members[b]
    labels = np.full(N, -1, dtype=np.int64)
    order = sorted(range(len(members)), key=lambda k: min(members[k]))
    for lab, k in enumerate(order):
        labels[members[k]] = lab
    return labels


def clustering(args, svec, cls_num, ahc_dis_th, cl_lst, sil_lst):
    """-> (clslab [n_chunks, num_speakers], cls_num): the non-silent vectors clustered on their Euclidean distances with the
    cannot-link pairs set clink_dis apart; silent slots carry the label cls_num (one past the clusters)"""
    svec = np.asarray(svec, dtype=np.float64)
    keep = np.setdiff1d(np.arange(len(svec)), np.asarray(sil_lst, dtype=np.int64))
    row = {int(o): r for r, o in enumerate(keep)}
    v = svec[keep]
    dist = np.sqrt(np.maximum(((v[:, None, :] - v[None, :, :]) ** 2).sum(-1), 0.0))
    for a, b in cl_lst:
        dist[row[a], row[b]] = dist[row[b], row[a]] = args.clink_dis
    labels = average_linkage(dist, n_clusters=cls_num, distance_threshold=ahc_dis_th)
    if cls_num is None:
        cls_num = int(labels.max()) + 1 if len(labels) else 0
    clslab = np.full(len(svec), cls_num, dtype=np.int64)
    clslab[keep] = labels
    return clslab.reshape(-1, args.num_speakers), cls_num


def merge_acti_clslab(args, acti, clslab, cls_num):
    """a cluster that holds several slots of one chunk (possible when the cannot-link distance is weak): the first of them
    takes the frame-wise maximum of all, the others become silent (zero activity, label cls_num).  In place."""
    for c, labs in enumerate(clslab):
        for lab in np.unique(labs[labs != cls_num]):
            slots = np.flatnonzero(labs == lab)
            if len(slots) > 1:
                acti[c][:, slots[0]] = acti[c][:, slots].max(axis=1)
                acti[c][:, slots[1:]] = 0.0
                labs[slots[1:]] = cls_num
    return acti, clslab


def stitching(args, acti, clslab, cls_num):
    """per chunk [frames, W - 1] with W = max(cls_num, num_speakers - 1) + 1: column l (the silent label's column left out)
    is the activity of the slot that carries label l in this chunk.  The chunk's slots are first padded with all-zero
    slots up to W, which take the labels no real slot uses, in ascending order; a label no slot carries shows the first silent
    slot (a padded, all-zero one unless a real slot is silent)."""
    n = args.num_speakers
    W = max(cls_num, n - 1) + 1
    out = []
    for c, a in enumerate(acti):
        labs = [int(l) for l in clslab[c]]
        used = [l for l in labs if l != cls_num]
        if len(set(used)) != len(used):
            raise ValueError("chunk %d: a label on two slots (merge_acti_clslab comes first)" % c)
        labs += sorted(set(range(W)) - set(labs))[:W - n]
        silent = [s for s, l in enumerate(labs) if l == cls_num]
        if not silent:
            raise ValueError("chunk %d: no silent slot" % c)
        a = np.asarray(a)
        padded = np.zeros((len(a), W), dtype=np.float64)
        padded[:, :n] = a
        src = np.full(W, silent[0], dtype=np.int64)
        for s, l in enumerate(labs):
            if l != cls_num:
                src[l] = s
        out.append(padded[:, np.delete(src, cls_num)])
    return out


def cluster(args, acti_list, svec, cls_num=None, info=None):
    """per-chunk activities (the new frames of each chunk) + the chunks x speakers vectors -> [total frames, speakers].  With
    fewer than two non-silent vectors (or fewer than a given cls_num) nothing is clustered and the activities pass through.
    info (a dict, optional) receives cl_lst, sil_lst, clslab (before the merge) and cls_num."""
    acti = [np.array(a, dtype=np.float64) for a in acti_list]
    cl_lst, sil_lst = get_cl_sil(args, acti, cls_num)
    if info is not None:
        info.update(cl_lst=cl_lst, sil_lst=sil_lst, clslab=None, cls_num=cls_num)
    if len(acti) * args.num_speakers - len(sil_lst) < (2 if cls_num is None else cls_num):
        return np.vstack(acti)
    clslab, cls_num = clustering(args, svec, cls_num, args.ahc_dis_th, cl_lst, sil_lst)
    if info is not None:
        info.update(clslab=clslab.copy(), cls_num=cls_num)
    acti, clslab = merge_acti_clslab(args, acti, clslab, cls_num)
    return np.vstack(stitching(args, acti, clslab, cls_num))


def medfilt_rows(a, k):
    """scipy.signal.medfilt(a, (k, 1)): median over k rows (k odd) per column, zeros beyond both ends"""
    a = np.asarray(a)
    if k % 2 != 1:
        raise ValueError("median=%d: the kernel size must be odd" % k)
    h = k // 2
    p = np.concatenate([np.zeros((h,) + a.shape[1:], a.dtype), a, np.zeros((h,) + a.shape[1:], a.dtype)])
    win = np.stack([p[i:i + len(a)] for i in range(k)])
    return np.sort(win, axis=0)[h]


def active_runs(column):
    """[(first frame, length)] of the runs of true values"""
    runs, t = [], 0
    for on, grp in itertools.groupby(bool(v) for v in column):
        n = sum(1 for _ in grp)
        if on:
            runs.append((t, n))
        t += n
    return runs


RTTM_LINE = "SPEAKER {:s} 1 {:7.2f} {:7.2f} <NA> <NA> {:s} <NA>"   # the reference's line: session, onset, duration, name


def make_rttm(args, cluster_data, frame_shift, subsampling, sampling_rate):
    """-> RTTM lines, speaker by speaker: activity above `threshold`, median filter over `median` frames (if > 1), one line
    per run of active frames; a frame is frame_shift * subsampling samples at sampling_rate; speakers are session_0, ..."""
    active = (np.asarray(cluster_data) > args.threshold).astype(np.int64)
    if args.median > 1:
        active = medfilt_rows(active, args.median)
    hop = frame_shift * subsampling
    return [RTTM_LINE.format(args.session, first * hop / sampling_rate, length * hop / sampling_rate, "%s_%d" % (args.session, spk))
            for spk in range(active.shape[1]) for first, length in active_runs(active[:, spk])]


def recording_chunks(model, n_samples16, chunk_size):
    """-> ([(start, end)] in 16 kHz samples, [new frames per chunk]).  The chunking is defined on the config's sr-rate samples
    (the reference reads its file at that rate and resamples each chunk to 16 kHz): the spans are scaled by 16000 / sr."""
    if model.sr <= 0 or 16000 % model.sr:
        raise NotImplementedError("sr=%r does not divide 16000" % (model.sr,))
    up = 16000 // model.sr
    spans, new_frames = chunk_recording(n_samples16 // up, chunk_size, model.frame_shift, model.subsampling)
    return [(s * up, e * up) for s, e in spans], new_frames


def predict(model, wav16, chunk_size, input_rate=16000):
    """a recording as ONE batch: wav16 1-D 16 kHz mono -> (acti_list: the new frames of every chunk [chunk_len, S], svec
    [chunks * S, E], chunk_len_list).  input_rate = model.sr (not 16000): the waveform is at the config's rate, as the
    reference reads it -- it is cut into chunks in sr-rate samples and the equal-length chunks go through ONE resample launch
    to 16 kHz (per chunk, not per recording: models.py:138,207 resamples each chunk batch, and the two differ round every seam)."""
    wav16 = torch.as_tensor(wav16)
    if wav16.dim() != 1:
        raise NotImplementedError("a waveform of shape %s: 16 kHz mono (1-D) is expected" % (tuple(wav16.shape),))
    if input_rate == 16000:
        spans, chunk_len_list = recording_chunks(model, len(wav16), chunk_size)
        chunks = [wav16[s:e] for s, e in spans]
    elif input_rate == model.sr:
        spans, chunk_len_list = chunk_recording(len(wav16), chunk_size, model.frame_shift, model.subsampling)
        chunks = _resample.resample(torch.stack([wav16[s:e] for s, e in spans]), input_rate, 16000)
    else:
        raise NotImplementedError("input_rate=%r: the waveform is either at 16000 Hz or at the model's sr=%r (then it is "
                                  "resampled chunk by chunk)" % (input_rate, model.sr))
    with torch.no_grad():
        acts, vecs = model.batch_estimate(chunks)
    acts, vecs = acts.float().cpu().numpy(), vecs.float().cpu().numpy()
    acti_list = [acts[i][len(acts[i]) - n:] for i, n in enumerate(chunk_len_list)]
    return acti_list, vecs.reshape(-1, vecs.shape[-1]), chunk_len_list


def diarize(model, wav16, chunk_size, args=None, sampling_rate=None, input_rate=16000):
    """16 kHz mono recording (or one at the model's sr with input_rate = model.sr, see predict) -> RTTM lines: one batched
    device call, then clustering, merge, stitching, median filter"""
    args = args or infer_args(num_speakers=model.n_speakers)
    acti_list, svec, _ = predict(model, wav16, chunk_size, input_rate)
    data = cluster(args, acti_list, svec)
    return make_rttm(args, data, model.frame_shift, model.subsampling, sampling_rate or model.sr)


# --------------------------------------------------------------------------------------------------------- command line
def load_config(path):
    """the reference's yaml (config/infer_est_nspk1.yaml) if `yaml` imports, else a json file of the same keys"""
    with open(path) as f:
        text = f.read()
    try:
        import yaml
    except ImportError:
        import json
        try:
            return json.loads(text)
        except ValueError:
            raise NotImplementedError("%s: PyYAML is not installed; give the config as a json file of the same keys" % path)
    return yaml.safe_load(text)


def read_wav(path, sr_model):
    """16-bit PCM mono at 16 kHz -> float32 tensor.  A file at the config's 8 kHz would need the reference's resampler."""
    from .kmeans import read_wav as _read
    wav, sr = _read(path)
    if sr != 16000:
        raise NotImplementedError("%s: sample rate %d; only 16 kHz input is taken (the reference resamples %d Hz audio with "
                                  "torchaudio's Resample, which is not built)" % (path, sr, sr_model))
    return torch.from_numpy(wav).float()


def read_recording(path, sr_model):
    """16-bit PCM mono at 16 kHz or at the config's sr -> (float32 tensor, rate); predict's input_rate takes the rate"""
    from .kmeans import read_wav as _read
    wav, sr = _read(path)
    if sr not in (16000, sr_model):
        raise NotImplementedError("%s: sample rate %d; the file must be at 16000 Hz or at the config's sr (%d Hz), which is "
                                  "resampled chunk by chunk as the reference does" % (path, sr, sr_model))
    return torch.from_numpy(wav).float(), sr


def load_pair(upstream_path, head_path, conf):
    """upstream checkpoint {'cfg', 'model'} + the reference's diarization checkpoint {'model': state dict} + its config"""
    from .wavlm import WavLM, WavLMConfig
    up = torch.load(upstream_path, map_location="cpu", weights_only=False)
    if not (isinstance(up, dict) and "cfg" in up and "model" in up):
        raise NotImplementedError("%s: only the standalone checkpoint dict {'cfg', 'model'} is loaded" % upstream_path)
    cfg = WavLMConfig(up["cfg"])
    wav = WavLM(cfg)
    wav.load_state_dict(up["model"])
    head = torch.load(head_path, map_location="cpu", weights_only=False)
    sd = fix_state_dict(head["model"] if isinstance(head, dict) and "model" in head else head)
    mconf = dict(conf["model"])
    mconf["all_n_speakers"] = sd["embed.weight"].shape[0]
    model = TransformerDiarization(upstream=wav, **mconf)
    model.load_state_dict(sd, strict=False)
    return model.cuda().eval()


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m unispeech_amd.diarization")
    ap.add_argument("upstream"); ap.add_argument("head"); ap.add_argument("config"); ap.add_argument("wav")
    ap.add_argument("--sil_spk_th", default=0.05, type=float)
    ap.add_argument("--ahc_dis_th", default=1.0, type=float)
    ap.add_argument("--clink_dis", default=1.0e4, type=float)
    ap.add_argument("--session", default="Anonymous")
    ap.add_argument("--out_rttm_file", default="out.rttm")
    ap.add_argument("--threshold", default=0.4, type=float)
    ap.add_argument("--median", default=25, type=int)
    ap.add_argument("--bf16", action="store_true", help="run upstream and head in bf16")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    conf = load_config(a.config)
    a.num_speakers = conf["dataset"]["num_speakers"]
    model = load_pair(a.upstream, a.head, conf)
    if a.bf16:
        model = model.to(torch.bfloat16)
    wav, rate = read_recording(a.wav, conf["model"].get("sr", 8000))
    with torch.no_grad():
        lines = diarize(model, wav.cuda(), conf["dataset"]["chunk_size"], a, conf["dataset"]["sampling_rate"], input_rate=rate)
    with open(a.out_rttm_file, "w") as f:
        f.write("".join(line + "\n" for line in lines))
    print("wrote %d segments to %s" % (len(lines), a.out_rttm_file))


if __name__ == "__main__":
    main()
