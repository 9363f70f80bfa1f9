"""Speaker embeddings on the device: ECAPA-TDNN over the upstream's layer states (csrc/spkhead.hip, ABI 23).

The inference path of the reference's downstreams/speaker_verification: `models/ecapa_tdnn.py` (`ECAPA_TDNN`,
`feature_selection="hidden_states"`), the hidden states `models/utils.py:49-56` collects through hooks, and
`verification.py`'s cosine score.
  * `ECAPA_TDNN` / `ECAPA_TDNN_SMALL` -- parameter and buffer names equal the reference's, so a released fine-tuned
    checkpoint loads as in verification.py:30-33 (`load_state_dict(ckpt["model"], strict=False)`); the upstream's keys sit
    under `feature_extract.model.*`.
  * `hidden_states(wavs)` -- the L+1 states straight from the encoder (no hooks, no [T, B, D] copies), one upstream call per
    distinct waveform length; `forward_states(states, lengths)` -- the head alone; `forward(wavs)` -- both.
  * `score(emb1, emb2)` -- cosine; `python -m unispeech_amd.speaker embed|verify UPSTREAM.pt HEAD.pt a.wav [b.wav]` (a file
    that is not at 16 kHz is resampled to it on the device, unispeech_amd/resample.py, as verification.py:46-49 does).
  * `ECAPA_TDNN(feat_dim=40, feat_type="fbank")` -- the reference's baseline without an upstream (verification.py's
    `ecapa_tdnn`): waveform -> log-mel filter bank on the device (unispeech_amd/fbank.py, one launch) -> the same head, layer 1
    a GEMM with K = 5 * 40; `... embed|verify --fbank HEAD.pt a.wav [b.wav]` on the command line.
Inference only (eval mode, BatchNorm running statistics, no gradients).  No CPU path and no eager fall-back for the kernels:
every tensor-sized step of the head is a libwavlm_hip.so entry point.  What torch does here is small and parameter- or
waveform-sized: the softmax of feature_weight, folding the BatchNorms and packing the Res2 weights (about 25 launches per call,
none under functional.frozen_parameters()), the waveform layer_norm of a `normalize` upstream, and copying each length group's
states into the padded batch.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from . import functional as F
from . import ops

__all__ = ["ECAPA_TDNN", "ECAPA_TDNN_SMALL", "score", "frame_count", "load_pair", "load_fbank"]

RES2_WIDTH = 64   # csrc/spkhead.hip: channels per Res2 split
RES2_SCALE = 8


# ------------------------------------------------------------------------------------------ parameter containers
# (the reference's module tree, ecapa_tdnn.py:14-160: names only -- none of these modules' forward is ever called)
class Conv1dReluBn(nn.Module):
    def __init__(self, cin, cout, kernel_size=1):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, kernel_size)
        self.bn = nn.BatchNorm1d(cout)


class Res2Conv1dReluBn(nn.Module):
    def __init__(self, channels, kernel_size, scale):
        super().__init__()
        self.width = channels // scale
        self.nums = scale - 1
        self.convs = nn.ModuleList([nn.Conv1d(self.width, self.width, kernel_size) for _ in range(self.nums)])
        self.bns = nn.ModuleList([nn.BatchNorm1d(self.width) for _ in range(self.nums)])


class SE_Connect(nn.Module):
    def __init__(self, channels, se_bottleneck_dim=128):
        super().__init__()
        self.linear1 = nn.Linear(channels, se_bottleneck_dim)
        self.linear2 = nn.Linear(se_bottleneck_dim, channels)


class SE_Res2Block(nn.Module):
    def __init__(self, channels, kernel_size, dilation, scale, se_bottleneck_dim):
        super().__init__()
        self.dilation = dilation
        self.Conv1dReluBn1 = Conv1dReluBn(channels, channels)
        self.Res2Conv1dReluBn = Res2Conv1dReluBn(channels, kernel_size, scale)
        self.Conv1dReluBn2 = Conv1dReluBn(channels, channels)
        self.SE_Connect = SE_Connect(channels, se_bottleneck_dim)


class AttentiveStatsPool(nn.Module):
    def __init__(self, in_dim, attention_channels=128):
        super().__init__()
        self.linear1 = nn.Conv1d(in_dim, attention_channels, kernel_size=1)
        self.linear2 = nn.Conv1d(attention_channels, in_dim, kernel_size=1)


class Upstream(nn.Module):
    """the reference's UpstreamExpert slot (models/utils.py:38-77): holds the model as `.model`"""

    def __init__(self, model):
        super().__init__()
        self.model = model


class MelBuffers(nn.Module):
    """the state-dict entries of the reference's `feature_extract` in fbank mode, a torchaudio MelSpectrogram:
    `spectrogram.window` [W] and `mel_scale.fb` [n_fft / 2 + 1, n_mels], so that key sets agree.  They hold what torchaudio
    builds (fbank.tables / fbank.mel_bank rounded to fp32); the kernel reads its own by-filter tables, never these."""

    def __init__(self, sr, n_fft, win_length, n_mels):
        super().__init__()
        from . import fbank as FB
        self.spectrogram, self.mel_scale = nn.Module(), nn.Module()
        t = FB.tables(sr, n_fft, win_length, n_mels)
        self.spectrogram.register_buffer("window", torch.from_numpy(t["window"].astype("float32")))
        self.mel_scale.register_buffer("fb", torch.from_numpy(FB.mel_bank(sr, n_fft, n_mels).astype("float32")))


def frame_count(n_samples, conv_feature_layers="[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2"):
    """frames the conv feature extractor yields for a waveform of n_samples"""
    n = int(n_samples)
    for _, k, s in eval(conv_feature_layers) if isinstance(conv_feature_layers, str) else conv_feature_layers:
        n = (n - k) // s + 1
    return n


def group_by_length(sizes):
    """{length: [indices]} in order of first appearance: one upstream call per distinct waveform length"""
    groups = {}
    for i, n in enumerate(sizes):
        groups.setdefault(int(n), []).append(i)
    return groups


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class UpstreamStates:
    """what every head over the upstream's layer states shares (this file's ECAPA_TDNN, diarization.TransformerDiarization):
    the model sits at self.feature_extract.model"""

    def _states_of(self, wav):
        """wav [b, n] (equal lengths) -> list of L + 1 tensors [b, T', D] in the reference's hook order (utils.py:49-56):
        the input of every encoder layer, then the encoder's output (after the final LayerNorm for a pre-LN stack)"""
        m = self.feature_extract.model
        x, _ = m._features(wav)
        enc = m.encoder
        L = len(enc.layers)
        _, results, _ = enc.extract_features(x, None, tgt_layer=L - 1)
        states = [r[0].transpose(0, 1) for r in results]   # [T, B, D] views of channel-last tensors: back to the tensors
        assert len(states) == L + 1
        if enc.layer_norm_first:
            ln = enc.layer_norm
            states[-1], _ = F.layer_norm(states[-1], ln.weight, ln.bias, ln.eps)
        return states

    def _wav_list(self, wavs):
        if isinstance(wavs, torch.Tensor):
            if wavs.dim() == 1:
                wavs = wavs.unsqueeze(0)
            if wavs.dim() != 2:
                raise NotImplementedError("input of shape %s: 16 kHz mono waveforms [B, T] or a list of 1-D tensors are "
                                          "expected" % (tuple(wavs.shape),))
            return list(wavs.unbind(0))
        wavs = [torch.as_tensor(w) for w in wavs]
        for w in wavs:
            if w.dim() != 1:
                raise NotImplementedError("a waveform of shape %s: 16 kHz mono (1-D) is expected; the reference resamples "
                                          "and down-mixes with torchaudio, which is not built" % (tuple(w.shape),))
        return wavs

    def _prepared_wavs(self, wavs):
        """fp32 on the upstream's device, layer-normed when its cfg.normalize is set (UpstreamExpert.forward,
        utils.py:59-60), then its dtype"""
        m = self.feature_extract.model
        p0 = next(m.parameters())
        normalize = bool(getattr(m.cfg, "normalize", False))
        prepared = []
        for w in wavs:
            w = w.to(device=p0.device, dtype=torch.float32)
            if normalize:
                w = torch.nn.functional.layer_norm(w, w.shape)
            prepared.append(w.to(p0.dtype))
        return prepared


class ECAPA_TDNN(UpstreamStates, nn.Module):
    """ecapa_tdnn.py:163-286 with feat_type = an upstream model and feature_selection="hidden_states", or feat_type="fbank".

    feat_dim: width D of the states; upstream: a unispeech_amd.wavlm.WavLM (its keys appear under feature_extract.model.*)
    or None for the head alone, in which case num_states (L + 1) must be given.
    feat_type="fbank": feat_dim is the number of mel filters (40 in verification.py); no upstream, no states and no
    feature_weight -- forward(wavs) computes the log-mel features itself (unispeech_amd/fbank.py)."""
    FBANK_N_FFT = 512   # ecapa_tdnn.py:180

    def __init__(self, feat_dim, channels=512, emb_dim=192, upstream=None, num_states=None, global_context_att=False,
                 feat_type="upstream", sr=16000, feature_selection="hidden_states", update_extract=False):
        super().__init__()
        if global_context_att:
            raise NotImplementedError("global_context_att=True (context mean / std concatenated in AttentiveStatsPool) is "
                                      "not built")
        if feat_type == "mfcc":
            raise NotImplementedError("feat_type=%r: the torchaudio mfcc front end is not built; the head runs on an upstream "
                                      "model's hidden states or on feat_type='fbank'" % feat_type)
        self.fbank = feat_type == "fbank"
        if self.fbank:
            from .fbank import MAX_MELS
            if not 1 <= int(feat_dim) <= MAX_MELS:
                raise NotImplementedError("feat_type='fbank' with feat_dim=%d: the fbank kernel takes 1 to %d mel filters "
                                          "(verification.py's ecapa_tdnn uses 40)" % (feat_dim, MAX_MELS))
            if upstream is not None or num_states not in (None, 1):
                raise ValueError("feat_type='fbank' takes neither an upstream nor num_states: the features are computed "
                                 "from the waveform")
        if update_extract:
            raise NotImplementedError("update_extract=True (fine-tuning the upstream through the head) is not built: "
                                      "inference only")
        if feature_selection != "hidden_states":
            raise NotImplementedError("feature_selection=%r: only 'hidden_states' is built" % (feature_selection,))
        if sr != 16000:
            raise NotImplementedError("sr=%r: input must be 16 kHz mono; the reference resamples with torchaudio, which is "
                                      "not built" % (sr,))
        if channels != RES2_WIDTH * RES2_SCALE:
            raise NotImplementedError("channels=%d: the Res2 kernel is built for 8 splits of 64 channels (channels=512)"
                                      % channels)
        self.feat_dim, self.sr = int(feat_dim), sr
        if self.fbank:
            self.feature_extract = MelBuffers(sr, self.FBANK_N_FFT, int(sr * 0.025), self.feat_dim)
            num_states = 1
        elif upstream is not None:
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
        if not self.fbank:   # ecapa_tdnn.py:203-205: the reference has none in fbank mode either
            self.feature_weight = nn.Parameter(torch.zeros(self.feat_num))
        self.instance_norm = nn.InstanceNorm1d(feat_dim)
        self.channels = [channels] * 4 + [1536]
        self.layer1 = Conv1dReluBn(feat_dim, channels, kernel_size=5)
        self.layer2 = SE_Res2Block(channels, 3, 2, RES2_SCALE, 128)
        self.layer3 = SE_Res2Block(channels, 3, 3, RES2_SCALE, 128)
        self.layer4 = SE_Res2Block(channels, 3, 4, RES2_SCALE, 128)
        self.conv = nn.Conv1d(channels * 3, self.channels[-1], kernel_size=1)
        self.pooling = AttentiveStatsPool(self.channels[-1], attention_channels=128)
        self.bn = nn.BatchNorm1d(self.channels[-1] * 2)
        self.linear = nn.Linear(self.channels[-1] * 2, emb_dim)

    # -- derived weight images ---------------------------------------------------------------------------------------
    def _head_tensors(self):
        up = "feature_extract."
        return [t for n, t in list(self.named_parameters()) + list(self.named_buffers()) if not n.startswith(up)]

    def _build_images(self):
        if self.fbank:
            im = {"w": torch.ones(1, dtype=torch.float32, device=self.layer1.conv.weight.device)}
        else:
            im = {"w": torch.softmax(self.feature_weight.float(), dim=-1).contiguous()}
        D = self.feat_dim
        im["l1_w"] = self.layer1.conv.weight.permute(0, 2, 1).reshape(-1, 5 * D).contiguous()  # [out, tap * D + in]
        blocks = [getattr(self, n) for n in ("layer2", "layer3", "layer4")]
        # every BatchNorm folded in one go (eval mode: scale = w / sqrt(var + eps), shift = b - mean * scale, fp32)
        bns = [self.layer1.bn]
        for blk in blocks:
            bns += [blk.Conv1dReluBn1.bn] + list(blk.Res2Conv1dReluBn.bns) + [blk.Conv1dReluBn2.bn]
        bns.append(self.bn)
        if len({b.eps for b in bns}) != 1:
            raise NotImplementedError("BatchNorm layers with different eps")
        cat = lambda name: torch.cat([getattr(b, name) for b in bns]).float()  # noqa: E731
        scale = cat("weight") / torch.sqrt(cat("running_var") + bns[0].eps)
        shift = cat("bias") - cat("running_mean") * scale
        sizes = [b.num_features for b in bns]
        folds = list(zip(scale.split(sizes), shift.split(sizes)))
        im["l1_bn"], im["bn"] = folds[0], folds[-1]
        k = 1
        for name, blk in zip(("layer2", "layer3", "layer4"), blocks):
            r2 = blk.Res2Conv1dReluBn
            n = r2.nums
            w = torch.stack([c.weight for c in r2.convs]).float()                 # [7, out, in, tap]
            # the seven 64-channel folds are adjacent in `scale` / `shift`: [7, 64] views, no copy
            o = sum(sizes[:k + 1])
            im[name] = dict(
                bn1=folds[k], bn2=folds[k + 1 + n],
                r2_w=w.permute(0, 3, 2, 1).contiguous(),                         # [7, tap, in, out]
                r2_b=torch.stack([c.bias for c in r2.convs]).float(),
                r2_scale=scale[o:o + n * r2.width].view(n, r2.width), r2_shift=shift[o:o + n * r2.width].view(n, r2.width))
            k += n + 2
        return im

    def _images(self):
        """BatchNorm folded to scale / shift, the k = 5 weight in tap-major rows, the Res2 weights packed: derived from the
        parameters per call, or kept under functional.frozen_parameters() (keyed by address and version of every head
        tensor; functional.invalidate_derived() drops them)"""
        return F.eval_derived(self._head_tensors(), "spk_images", self._build_images, inference=True)

    def load_state_dict(self, *a, **k):
        F.invalidate_derived()
        return super().load_state_dict(*a, **k)

    # -- checks --------------------------------------------------------------------------------------------------------
    def _inference_only(self):
        if self.training:
            raise NotImplementedError("forward in training mode (update_extract / head training: BatchNorm batch statistics, "
                                      "gradients) is not built: call .eval()")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("forward with gradients required is not built (inference only): run under "
                                      "torch.no_grad()")

    # -- upstream: UpstreamStates ---------------------------------------------------------------------------------------
    def hidden_states(self, wavs):
        """list of 1-D waveforms or [B, T] -> (states: L + 1 tensors [B, T'max, D], lengths: frames per utterance, or None
        when all are equal).  The waveform is layer-normed first when the upstream's cfg.normalize is set
        (UpstreamExpert.forward, utils.py:59-60).  Unequal lengths: one upstream call per distinct length (what one
        verification.py call per file computes); absent frames are zero."""
        self._inference_only()
        if self.fbank:
            raise ValueError("an fbank model has no upstream and no hidden states: use forward or fbank_features")
        if not hasattr(self, "feature_extract"):
            raise ValueError("this head was built without an upstream: use forward_states")
        m = self.feature_extract.model
        wavs = self._wav_list(wavs)
        prepared = self._prepared_wavs(wavs)
        groups = group_by_length(len(w) for w in prepared)
        with torch.no_grad():
            if len(groups) == 1:
                return self._states_of(torch.stack(prepared)), None
            layers = getattr(m.cfg, "conv_feature_layers")
            frames = [frame_count(len(w), layers) for w in prepared]
            Tm = max(frames)
            out = None
            for n, idx in groups.items():
                st = self._states_of(torch.stack([prepared[i] for i in idx]))
                if out is None:
                    out = [s.new_zeros((len(prepared), Tm, s.shape[-1])) for s in st]
                for o, s in zip(out, st):
                    o[idx, :s.shape[1]] = s
            return out, frames

    # -- head ----------------------------------------------------------------------------------------------------------
    def forward_states(self, states, lengths=None, intermediates=None):
        """states: L + 1 tensors [B, T', D] (or one [L + 1, B, T', D]) in the head's dtype, channel-last, read in place;
        lengths: frames per utterance (absent frames never reach an output).  Returns embeddings [B, emb_dim].
        intermediates (a dict, optional) receives `normed`, `out2_mean`, `out4_mean`, `pooled` for the tests."""
        self._inference_only()
        if self.fbank:
            raise ValueError("an fbank model has no hidden states: use forward")
        if isinstance(states, torch.Tensor):
            states = list(states.unbind(0))
        states = [s if s.stride(-1) == 1 and s.stride(1) >= s.shape[2] else s.contiguous() for s in states]
        if len(states) != self.feat_num:
            raise ValueError("%d states given, feature_weight holds %d" % (len(states), self.feat_num))
        s0 = states[0]
        dev, dtype = ops._dev(s0), s0.dtype
        B, T, D = s0.shape
        pd = self.layer1.conv.weight.dtype
        if D != self.feat_dim or any(s.shape != s0.shape or s.dtype != dtype or s.device != dev for s in states):
            raise ValueError("states must share one shape [B, T', %d], dtype and device" % self.feat_dim)
        if dtype != pd:
            raise TypeError("states are %s but the head's parameters are %s" % (dtype, pd))
        dt = ops.dt(s0)
        len_t = None
        if lengths is not None:
            lt = torch.as_tensor(lengths)
            if not lt.is_cuda:
                if lt.numel() != B or int(lt.min()) < 1 or int(lt.max()) > T:
                    raise ValueError("lengths must hold %d frame counts in [1, %d]" % (B, T))
            len_t = lt.to(device=dev, dtype=torch.int32).contiguous()
        with torch.no_grad():
            return self._head(states, len_t, B, T, D, dev, dtype, dt, intermediates)

    def _head(self, states, len_t, B, T, D, dev, dtype, dt, inter, sdt=None):
        """dtype / dt: the head's; sdt: the states' dtype code when it differs (fp32 log-mel features into a bf16 head)"""
        L = _lib.lib()
        sdt = dt if sdt is None else sdt
        st = ops.stream
        im = self._images()
        n = len(states)
        lp = _p(len_t)
        new = lambda *shape: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
        ch = self.channels[0]
        cat_c = 3 * ch

        # layer mix + instance norm into a tensor with the k = 5 convolution's two zero frames on each side
        xp = new(B, T + 4, D)
        ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in states])
        sb = (C.c_int64 * n)(*[s.stride(0) for s in states])
        stt = (C.c_int64 * n)(*[s.stride(1) for s in states])
        _lib.check(L.wavlm_spk_mix_norm(ptrs, sb, stt, n, sdt, _p(im["w"]), lp, B, T, D, ops.ptr(xp, 2 * D), dt, (T + 4) * D, D, 2,
                                        0.0 if self.fbank else 1e-6, self.instance_norm.eps, st()), "wavlm_spk_mix_norm")
        if inter is not None:
            inter["normed"] = xp[:, 2:T + 2]

        def rowact(x, ldx, C_, act, fold, mean=None, x_off=0):
            sc, sh = fold if fold is not None else (None, None)
            _lib.check(L.wavlm_spk_rowact(ops.ptr(x, x_off), dt, T * ldx, ldx, ops.ptr(x, x_off), dt, T * ldx, ldx, B, T, C_, act,
                                          _p(sc), _p(sh), lp, _p(mean), st()), "wavlm_spk_rowact")

        # layer1: k = 5 convolution = GEMM over overlapping rows of the padded tensor, then ReLU + BatchNorm
        h = new(B, T, ch)
        ops.gemm(xp, im["l1_w"], h, T, ch, 5 * D, lda=D, ldb=5 * D, ldc=ch, batch=(B, 1), sA=((T + 4) * D, 0), sC=(T * ch, 0),
                 bias=self.layer1.conv.bias)
        rowact(h, ch, ch, 0, im["l1_bn"])

        cat = new(B, T, cat_c)      # out2 | out3 | out4: the blocks write their slices, torch.cat never runs
        a, r = new(B, T, ch), new(B, T, ch)
        mean = torch.empty((B, ch), dtype=torch.float32, device=dev)
        ws_bytes = L.wavlm_spk_se_workspace_bytes(B, ch)
        ws = ops.workspace(dev, ws_bytes, "spk")
        prev, prev_off, prev_ld = h, 0, ch
        for i, name in enumerate(("layer2", "layer3", "layer4")):
            blk, bi = getattr(self, name), im[name]
            c1, c2, se = blk.Conv1dReluBn1.conv, blk.Conv1dReluBn2.conv, blk.SE_Connect
            ops.gemm(prev, c1.weight, a, B * T, ch, ch, lda=prev_ld, ldb=ch, ldc=ch, a_off=prev_off, bias=c1.bias)
            rowact(a, ch, ch, 0, bi["bn1"])
            _lib.check(L.wavlm_spk_res2(_p(a), dt, T * ch, ch, _p(r), dt, T * ch, ch, B, T, ch, blk.dilation, _p(bi["r2_w"]),
                                        _p(bi["r2_b"]), _p(bi["r2_scale"]), _p(bi["r2_shift"]), lp, st()), "wavlm_spk_res2")
            ops.gemm(r, c2.weight, a, B * T, ch, ch, lda=ch, ldb=ch, ldc=ch, bias=c2.bias)
            rowact(a, ch, ch, 0, bi["bn2"], mean=mean)
            _lib.check(L.wavlm_spk_se_residual(_p(a), dt, T * ch, ch, _p(mean), _p(se.linear1.weight), _p(se.linear1.bias),
                                               _p(se.linear2.weight), _p(se.linear2.bias), dt, ops.ptr(prev, prev_off), dt,
                                               T * prev_ld, prev_ld, ops.ptr(cat, i * ch), dt, T * cat_c, cat_c, B, T, ch,
                                               se.linear1.out_features, lp, _p(ws), ws_bytes, st()), "wavlm_spk_se_residual")
            prev, prev_off, prev_ld = cat, i * ch, cat_c
        if inter is not None:
            div = (len_t.float() if len_t is not None else torch.full((B,), float(T), device=dev)).view(B, 1)
            inter["out2_mean"] = cat[:, :, :ch].float().sum(1) / div
            inter["out4_mean"] = cat[:, :, 2 * ch:].float().sum(1) / div

        # 1536 -> 1536, ReLU; the two pooling projections; pooling + BatchNorm; the embedding
        cc = self.channels[-1]
        y = new(B, T, cc)
        ops.gemm(cat, self.conv.weight, y, B * T, cc, cat_c, lda=cat_c, ldb=cat_c, ldc=cc, bias=self.conv.bias)
        rowact(y, cc, cc, 0, None)
        p1, p2 = self.pooling.linear1, self.pooling.linear2
        ac = p1.out_channels
        t1 = new(B, T, ac)
        ops.gemm(y, p1.weight, t1, B * T, ac, cc, lda=cc, ldb=cc, ldc=ac, bias=p1.bias)
        rowact(t1, ac, ac, 1, None)
        lg = new(B, T, cc)
        ops.gemm(t1, p2.weight, lg, B * T, cc, ac, lda=ac, ldb=ac, ldc=cc, bias=p2.bias)
        pooled = new(B, 2 * cc)
        raw = torch.empty((B, 2 * cc), dtype=torch.float32, device=dev) if inter is not None else None
        _lib.check(L.wavlm_spk_asp(_p(y), dt, T * cc, cc, _p(lg), dt, T * cc, cc, B, T, cc, lp, _p(im["bn"][0]), _p(im["bn"][1]),
                                   _p(raw), _p(pooled), dt, st()), "wavlm_spk_asp")
        if inter is not None:
            inter["pooled"] = raw
        E = self.linear.out_features
        emb = new(B, E)
        ops.gemm(pooled, self.linear.weight, emb, B, E, 2 * cc, lda=2 * cc, ldb=2 * cc, ldc=E, bias=self.linear.bias)
        return emb

    # -- fbank front end ---------------------------------------------------------------------------------------------------
    def fbank_features(self, wavs):
        """list of 1-D 16 kHz mono waveforms (float, or int16 PCM) or [B, T] -> (log-mel features fp32 [B, Tmax, feat_dim],
        frames per utterance): ecapa_tdnn.py:253 (MelSpectrogram + 1e-6) and :257 (log), one launch for the whole list"""
        from . import fbank as FB
        if not self.fbank:
            raise ValueError("this model runs on an upstream's hidden states, not on fbank features")
        dev = self.layer1.conv.weight.device
        wavs = [w.to(device=dev, dtype=torch.int16 if w.dtype == torch.int16 else torch.float32) for w in self._wav_list(wavs)]
        if len({w.dtype for w in wavs}) != 1:
            raise ValueError("waveforms of one call share a dtype (float or int16 PCM)")
        W, S, P = FB.geometry(self.sr, self.FBANK_N_FFT)
        frames = [FB.frames(len(w), S, P) for w in wavs]
        if min(frames) < 1:
            raise ValueError("a waveform of %d samples: the reflection at its ends needs more than %d"
                             % (min(len(w) for w in wavs), P // 2))
        x = torch.stack(wavs) if len({len(w) for w in wavs}) == 1 else wavs
        return FB.fbank(x, sr=self.sr, n_mels=self.feat_dim, n_fft=P, win_length=W, hop_length=S), frames

    def _forward_fbank(self, wavs, intermediates=None):
        self._inference_only()
        with torch.no_grad():
            feats, frames = self.fbank_features(wavs)
            B, T, D = feats.shape
            w0 = self.layer1.conv.weight
            len_t = None
            if min(frames) != T:
                len_t = torch.tensor(frames, dtype=torch.int32).to(w0.device)
            # the 1e-6 is inside the log already: one fp32 "state", weight 1, add 0, normed into the head's dtype
            return self._head([feats], len_t, B, T, D, w0.device, w0.dtype, ops.dt(w0), intermediates, sdt=_lib.F32)

    def forward(self, wavs, intermediates=None):
        """list of 1-D 16 kHz mono waveforms or [B, T] -> embeddings [B, emb_dim] (ecapa_tdnn.py:273-286)"""
        if self.fbank:
            return self._forward_fbank(wavs, intermediates)
        states, frames = self.hidden_states(wavs)
        return self.forward_states(states, frames, intermediates)


def ECAPA_TDNN_SMALL(feat_dim, emb_dim=256, **kwargs):
    """ecapa_tdnn.py:289-291: channels 512"""
    return ECAPA_TDNN(feat_dim=feat_dim, channels=512, emb_dim=emb_dim, **kwargs)


def score(emb1, emb2, eps=1e-8):
    """verification.py:61: F.cosine_similarity along the last dimension"""
    return torch.nn.functional.cosine_similarity(emb1.float(), emb2.float(), dim=-1, eps=eps)


# --------------------------------------------------------------------------------------------------------- command line
def read_wav_16k(path):
    """16-bit PCM, 16 kHz (kmeans.read_wav; channels averaged) -> float32 tensor; any other rate is refused"""
    from .kmeans import read_wav
    wav, sr = read_wav(path)
    if sr != 16000:
        raise NotImplementedError("%s: sample rate %d; only 16 kHz input is taken (the reference resamples with torchaudio's "
                                  "Resample, which is not built)" % (path, sr))
    return torch.from_numpy(wav).float()


def read_wav(path):
    """16-bit PCM at any rate (kmeans.read_wav; channels averaged) -> (float32 tensor, sample rate)"""
    from .kmeans import read_wav as _read
    wav, sr = _read(path)
    return torch.from_numpy(wav).float(), sr


def to_16k(wav, rate):
    """verification.py:46-49: a file that is not at 16 kHz is resampled to it, here on the device (resample.py)"""
    from .resample import resample
    return resample(wav.cuda(), rate, 16000)


def load_pair(upstream_path, head_path, emb_dim=256):
    """upstream checkpoint {'cfg', 'model'} + head checkpoint {'model': state dict} (the reference's
    fine-tuned file: head keys, optionally feature_extract.model.* as well) -> ECAPA_TDNN_SMALL on the device, eval mode"""
    from .wavlm import WavLM, WavLMConfig
    up = torch.load(upstream_path, map_location="cpu", weights_only=False)
    if not (isinstance(up, dict) and "cfg" in up and "model" in up):
        raise NotImplementedError("%s: only the standalone checkpoint dict {'cfg', 'model'} is loaded" % upstream_path)
    cfg = WavLMConfig(up["cfg"])
    wav = WavLM(cfg)
    wav.load_state_dict(up["model"])
    model = ECAPA_TDNN_SMALL(cfg.encoder_embed_dim, emb_dim=emb_dim, upstream=wav)
    head = torch.load(head_path, map_location="cpu", weights_only=False)
    model.load_state_dict(head["model"] if isinstance(head, dict) and "model" in head else head, strict=False)
    return model.cuda().eval()


def load_fbank(head_path, emb_dim=256, feat_dim=40):
    """head checkpoint {'model': state dict} (the reference's released ECAPA-TDNN file) -> ECAPA_TDNN_SMALL(feat_dim,
    feat_type='fbank') on the device, eval mode; loaded with strict=False as verification.py:30-33 does"""
    model = ECAPA_TDNN_SMALL(feat_dim, emb_dim=emb_dim, feat_type="fbank")
    head = torch.load(head_path, map_location="cpu", weights_only=False)
    head = head["model"] if isinstance(head, dict) and "model" in head else head
    # the front end's own tables stay: the kernel is built from them, not from the file's
    model.load_state_dict({k: v for k, v in head.items() if not k.startswith("feature_extract.")}, strict=False)
    return model.cuda().eval()


def parse_args(argv=None):
    """embed|verify UPSTREAM.pt HEAD.pt wavs...; with --fbank (verification.py's ecapa_tdnn: no upstream) HEAD.pt wavs..."""
    import argparse
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    fb = "--fbank" in argv
    ap = argparse.ArgumentParser(prog="python -m unispeech_amd.speaker")
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("embed", help="print the embedding of each wav file")
    if not fb:
        p.add_argument("upstream")
    p.add_argument("head"); p.add_argument("wavs", nargs="+")
    p = sub.add_parser("verify", help="verification.py: cosine score of two wav files")
    if not fb:
        p.add_argument("upstream")
    p.add_argument("head"); p.add_argument("wav1"); p.add_argument("wav2")
    for q in sub.choices.values():
        q.add_argument("--emb_dim", default=256, type=int)
        q.add_argument("--bf16", action="store_true", help="run upstream and head in bf16")
        q.add_argument("--fbank", action="store_true", help="the ECAPA-TDNN baseline on 40 log-mel filters: no upstream argument")
    a = ap.parse_args(argv)
    if fb:
        a.upstream = None
    return a


def main(argv=None):
    a = parse_args(argv)
    paths = a.wavs if a.cmd == "embed" else [a.wav1, a.wav2]
    wavs = [read_wav(p) for p in paths]
    model = load_fbank(a.head, a.emb_dim) if a.fbank else load_pair(a.upstream, a.head, a.emb_dim)
    if a.bf16:
        model = model.to(torch.bfloat16)
    with torch.no_grad():
        emb = model([to_16k(w, sr) for w, sr in wavs])
    if a.cmd == "embed":
        for p, e in zip(paths, emb.float().cpu()):
            print(p, " ".join("%.6f" % v for v in e.tolist()))
    else:
        sim = score(emb[0:1], emb[1:2])
        print("The similarity score between two audios is {:.4f} (-1.0, 1.0).".format(sim[0].item()))


if __name__ == "__main__":
    main()
