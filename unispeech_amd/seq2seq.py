"""Seq2seq ASR on the device, inference only (csrc/s2s.hip, additive to ABI 30): the reference's `wav2vec_seq2seq`
(src/fairseq/models/wav2vec/wav2vec2_asr.py:215-643: Wav2VecEncoder + an autoregressive TransformerDecoder that attends to the
encoder's frames) decoded the way `SequenceGenerator` (src/fairseq/sequence_generator.py) with `BeamSearch` (search.py) decodes it
-- what examples/speech_recognition/infer.py falls back to when no --w2l-decoder is given.

  Seq2SeqConfig      the decoder_* fields of Wav2Vec2Seq2SeqConfig; every other option is one of Wav2Vec2AsrConfig's and goes through
                     ctc.py's option split (ctc.EncoderCtc goes on refusing the decoder_* fields).
  Wav2Vec2Seq2Seq    parameter names equal the reference's, so `load_state_dict(strict=True)` takes its state dict as it stands:
                     encoder.w2v_model.*, encoder.proj.{weight, bias} (only when decoder_embed_dim differs from the encoder's
                     width), decoder.embed_tokens.weight, decoder.embed_positions.{weight | _float_tensor},
                     decoder.layers.N.{self_attn, encoder_attn}.{q, k, v, out}_proj, .{self_attn, encoder_attn, final}_layer_norm,
                     .fc1, .fc2, decoder.layer_norm (decoder_normalize_before), decoder.embed_out (unless
                     share_decoder_input_output_embed).  The reference builds the embedding decoder_embed_dim wide, so its
                     project_in_dim never exists; its layers' activation is ReLU (the config has no activation_fn).
                     Refused by name: a head width other than 32 or 64 -- which includes the reference's default of 4 heads at
                     768 --, train(), inputs that require gradients, decoder_layerdrop in training.
  forward            (source, padding_mask, prev_output_tokens) -> teacher-forced logits [B, T, V] (fp32).  The reference's own
                     Wav2Vec2Seq2SeqModel.forward hands the decoder a batch-first encoder output (tbc=False) and cannot run
                     unless B == Ts; this is the model as SequenceGenerator runs it (encoder.forward, then decoder.forward).
  generate           beam search on the device.  The encoder runs once, its K | V once per layer (one wavlm_gemm against the
                     stacked k_proj / v_proj); a step is B * beam rows through wavlm_gemm / wavlm_layernorm_fwd / wavlm_act_fwd,
                     wavlm_attn_step over a KV cache shaped as the tree of hypotheses (nothing is reordered), wavlm_attn_cross_fwd
                     with the rows of a sentence sharing one pass over its frames, one wavlm_gemm onto the vocabulary and
                     wavlm_beam_step.  The shapes are the same at every step; finished sentences' rows are skipped through
                     `lengths`.  Inside the loop the host reads one int32 -- the count of finished sentences -- every
                     READ_EVERY steps (read_device counts the reads: Wav2Vec2Seq2Seq.loop_reads).
                     Refused by name: prefix_tokens, constraints, sampling, match_source_len, ensembles -- and lm_model,
                     lm_weight and no_repeat_ngram_size, which sequence_generator.SequenceGenerator takes.
  search             generate() behind the encoder.  Keyword-only lm_model= (a TransformerLM over the same dictionary), lm_weight=
                     and no_repeat_ngram_size= turn the step into wavlm_beam_step_fused: the LM runs incrementally over caches
                     of its own shaped as the same tree (wavlm_attn_step with the search's slots, ancestors and lengths), one
                     wavlm_gemm gives its logits, and the step adds lm_weight * log_softmax before the NaN rule
                     (sequence_generator.py:338-346; a plain log-softmax: FairseqLM's unk rule is not SequenceGenerator's) and
                     bans repeated n-grams from the tree's histories (ngram_repeat_block.py).  No host read is added.  Taken
                     literally: lm_weight 0 against an LM entry of -inf is NaN, hence -inf; no_repeat_ngram_size 1 bans
                     every token of the history, eos (the row's first token) included.
  decoder_reference, beam_step_reference, beam_search_reference, generate_reference
                     the same in float64 torch on the CPU: the specification.  Host tensors go through these; there is no CPU
                     build of the kernels.
  python -m unispeech_amd.seq2seq decode CKPT DICT audio.wav ... [--beam N --max-len-a A --max-len-b B --lenpen P --nbest N]
  python -m unispeech_amd.seq2seq score CKPT DICT MANIFEST.tsv LABELS.ltr [--results DIR]
      either with [--lm LM.pt --lm-weight W] [--no-repeat-ngram-size N]: LM.pt is a TransformerLM checkpoint over the same DICT

Ties: candidates are ordered by (score descending, beam row * V + token ascending).  torch.topk leaves ties open.
bf16 and fp32 (parity) modes: `.to(torch.bfloat16)` as the other heads have it; the search itself is fp32 in both.
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn

from .transformer_lm import _attend64, _lin64, _ln64, sinusoidal_table

__all__ = ["Seq2SeqConfig", "Wav2Vec2Seq2Seq", "decoder_reference", "beam_step_reference", "beam_search_reference",
           "generate_reference", "ngram_banned", "read_device"]

READ_EVERY = 8                         # steps between two reads of the finished counter
GENERATE_REFUSED = ("prefix_tokens", "constraints", "sampling", "sampling_topk", "sampling_topp", "match_source_len",
                    "no_repeat_ngram_size", "lm_model", "lm_weight", "diverse_beam_groups", "diversity_rate", "models", "ensemble")
FUSION_OPTIONS = ("lm_model", "lm_weight", "no_repeat_ngram_size")     # built, behind sequence_generator.SequenceGenerator


class Seq2SeqConfig:
    """the decoder_* fields of Wav2Vec2Seq2SeqConfig (names and defaults) from a dict, a Namespace or keywords; a fairseq `cfg`
    with a `model` group is unwrapped.  `encoder_options`: what is left, for ctc.py's option split."""
    DEFAULTS = dict(decoder_embed_dim=768, decoder_ffn_embed_dim=3072, decoder_layers=6, decoder_layerdrop=0.0,
                    decoder_attention_heads=4, decoder_learned_pos=False, decoder_normalize_before=False,
                    no_token_positional_embeddings=False, decoder_dropout=0.0, decoder_attention_dropout=0.0,
                    decoder_activation_dropout=0.0, max_target_positions=2048, share_decoder_input_output_embed=False)
    IGNORED = ("autoregressive", "_name", "arch", "w2v_args", "w2v_path", "data", "normalize", "no_pretrained_weights")

    def __init__(self, options=None, **kw):
        if options is not None and not isinstance(options, dict):
            options = dict(vars(options))
        options = dict(options or {})
        if isinstance(options.get("model"), dict) or hasattr(options.get("model"), "__dict__"):
            m = options["model"]
            options = dict(m if isinstance(m, dict) else vars(m))
        options.update(kw)
        for k, v in self.DEFAULTS.items():
            setattr(self, k, options.pop(k, v))
        for k in self.IGNORED:
            options.pop(k, None)
        self.encoder_options = options

    def as_dict(self):
        return {k: getattr(self, k) for k in self.DEFAULTS}


# ------------------------------------------------------------------------------------------------ parameter containers
class _Attention(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(D, D) for _ in range(4))


class _Layer(nn.Module):
    def __init__(self, D, F):
        super().__init__()
        self.self_attn = _Attention(D)
        self.self_attn_layer_norm = nn.LayerNorm(D)
        self.encoder_attn = _Attention(D)
        self.encoder_attn_layer_norm = nn.LayerNorm(D)
        self.fc1, self.fc2 = nn.Linear(D, F), nn.Linear(F, D)
        self.final_layer_norm = nn.LayerNorm(D)


class _Sinusoidal(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("_float_tensor", torch.zeros(1))


class _Decoder(nn.Module):
    def __init__(self, cfg, V, pad):
        super().__init__()
        D = cfg.decoder_embed_dim
        self.embed_tokens = nn.Embedding(V, D, pad)
        if not cfg.no_token_positional_embeddings:
            self.embed_positions = (nn.Embedding(cfg.max_target_positions + pad + 1, D, pad) if cfg.decoder_learned_pos
                                    else _Sinusoidal())
        self.layers = nn.ModuleList([_Layer(D, cfg.decoder_ffn_embed_dim) for _ in range(cfg.decoder_layers)])
        if not cfg.share_decoder_input_output_embed:
            self.embed_out = nn.Parameter(torch.empty(V, D))
            nn.init.normal_(self.embed_out, mean=0, std=D ** -0.5)
        if cfg.decoder_normalize_before:
            self.layer_norm = nn.LayerNorm(D)

    def output_weight(self):
        return self.embed_out if hasattr(self, "embed_out") else self.embed_tokens.weight


def _make_encoder(w2v_model, D, opts):
    from . import ctc

    class _Encoder(ctc._Encoder):
        """Wav2VecEncoder (wav2vec2_asr.py:312-439): w2v_model, and proj only onto a decoder of another width"""

        def __init__(self, w2v_model, D, opts):
            super().__init__(w2v_model, D, opts)
            if w2v_model.cfg.encoder_embed_dim == D:
                self.proj = None

        def forward(self, source, padding_mask=None, **kwargs):
            """-> (features [B, Ts, D] after proj, padding mask [B, Ts] or None)"""
            from . import ops
            res = self.w2v_model.extract_features(source=source, padding_mask=padding_mask, mask=False)
            x, pm = (res["x"], res["padding_mask"]) if isinstance(res, dict) else res
            if self.proj is not None:
                B, Ts, d = x.shape
                x = x.reshape(B * Ts, d).contiguous()
                y = torch.empty((B * Ts, self.proj.weight.shape[0]), dtype=x.dtype, device=x.device)
                ops.gemm(x, self.proj.weight, y, B * Ts, y.shape[1], d, lda=d, ldb=d, ldc=y.shape[1], bias=self.proj.bias)
                x = y.view(B, Ts, -1)
            return x, pm

    return _Encoder(w2v_model, D, opts)


def read_device(t):
    """every device-to-host read generate() makes inside its loop goes through here (Wav2Vec2Seq2Seq.loop_reads counts them)"""
    return t.cpu()


class Wav2Vec2Seq2Seq(nn.Module):
    """w2v_model: a pre-training model of this package after remove_pretraining_modules(); vocab: the target dictionary's size;
    pad / eos / unk: its special ids (fairseq's Dictionary: 1, 2, 3); cfg: a Seq2SeqConfig (or what it takes)."""

    def __init__(self, w2v_model, vocab, cfg=None, pad=1, eos=2, unk=3, **options):
        super().__init__()
        from . import ctc
        cfg = cfg if isinstance(cfg, Seq2SeqConfig) else Seq2SeqConfig(cfg, **options)
        D, H = cfg.decoder_embed_dim, cfg.decoder_attention_heads
        if D % H or D // H not in (32, 64):
            raise NotImplementedError("decoder_embed_dim=%d / decoder_attention_heads=%d: the attention kernels are built for "
                                      "heads 32 or 64 wide" % (D, H))
        opts, _ = ctc._split_options(cfg.encoder_options, allow_overrides=False)
        for name in ("final_proj", "label_embs_concat"):
            if getattr(w2v_model, name, None) is not None:
                raise ValueError("call remove_pretraining_modules() on the wrapped model first (%s is still there)" % name)
        self.cfg, self.vocab, self.pad, self.eos, self.unk = cfg, int(vocab), int(pad), int(eos), int(unk)
        self.embed_scale = math.sqrt(D)
        self.encoder = _make_encoder(w2v_model, D, opts)
        self.decoder = _Decoder(cfg, self.vocab, self.pad)
        self._image_cache = None
        self.loop_reads = self.loop_steps = 0                        # of the last search: host reads inside the loop, steps run
        self.eval()

    # -- loading ---------------------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, w2v_cfg, vocab, cfg=None, *, arch="wav2vec2", task_cfg=None, state_dict=None, pad=1, eos=2, unk=3, **options):
        """Wav2VecEncoder.__init__ + build_decoder: the pre-training model built from its config (ctc.EncoderCtc.build's recipe:
        overrides applied, pre-training modules removed), wrapped; state_dict: the whole model's, strict"""
        from . import ctc
        cfg = cfg if isinstance(cfg, Seq2SeqConfig) else Seq2SeqConfig(cfg, **options)
        inner = ctc.EncoderCtc.build(w2v_cfg, 8, arch=arch, task_cfg=task_cfg, **cfg.encoder_options).w2v_encoder.w2v_model
        cfg.encoder_options = {k: v for k, v in cfg.encoder_options.items() if k in ctc.OPTIONS}
        model = cls(inner, vocab, cfg, pad=pad, eos=eos, unk=unk)
        if state_dict is not None:
            model.load_state_dict(state_dict, strict=True)
        return model

    @classmethod
    def from_checkpoint(cls, path, dictionary):
        """{"cfg" | "args", "model"} -> the model on the CPU in fp32.  The pre-training config is taken as EncoderCtc.build takes
        it: cfg["w2v_args"] (a dict of the pre-training model's fields, or a {"model": ...} group), else the checkpoint
        cfg["w2v_path"] names ({"cfg" | "args"} of the pre-training run).  "arch": "wav2vec2" (default) or "wavlm"."""
        ck = torch.load(path, map_location="cpu", weights_only=False)
        if not (isinstance(ck, dict) and "model" in ck and (ck.get("cfg") is not None or ck.get("args") is not None)):
            raise NotImplementedError("%s: only a checkpoint dict {'cfg' | 'args', 'model'} is loaded" % path)
        from . import ctc
        opts = ck["cfg"] if ck.get("cfg") is not None else ck["args"]
        opts = dict(opts if isinstance(opts, dict) else vars(opts))
        if isinstance(opts.get("model"), dict) or hasattr(opts.get("model"), "__dict__"):
            m = opts["model"]
            opts = dict(m if isinstance(m, dict) else vars(m))
        known = set(Seq2SeqConfig.DEFAULTS) | set(ctc.OPTIONS) | set(ctc.OVERRIDES) | {"w2v_args", "w2v_path", "normalize"}
        opts = {k: v for k, v in opts.items() if k in known}           # a fairseq cfg carries fields of other components too
        w2v = opts.get("w2v_args")
        if w2v is None:
            if not opts.get("w2v_path"):
                raise ValueError("%s: neither w2v_args nor w2v_path says how the encoder is built" % path)
            pre = torch.load(opts["w2v_path"], map_location="cpu", weights_only=False)
            w2v = pre["cfg"] if pre.get("cfg") is not None else pre["args"]
        w2v = dict(w2v if isinstance(w2v, dict) else vars(w2v))
        if isinstance(w2v.get("model"), dict) or hasattr(w2v.get("model"), "__dict__"):
            m = w2v["model"]
            w2v = dict(m if isinstance(m, dict) else vars(m))
        arch = ck.get("arch", "wav2vec2")
        if arch == "wav2vec2":
            from .wav2vec2 import Wav2Vec2Config as Cfg
        else:
            from .pretrain import WavLMPretrainConfig as Cfg
        w2v_cfg = Cfg(**{k: v for k, v in w2v.items() if k in Cfg.__dataclass_fields__})
        model = cls.build(w2v_cfg, len(dictionary), Seq2SeqConfig(opts), arch=arch, state_dict=ck["model"], pad=dictionary.pad(),
                          eos=dictionary.eos(), unk=dictionary.unk())
        model.normalize = bool(ck.get("normalize", opts.get("normalize", False)))
        return model

    def load_state_dict(self, state_dict, strict=True):
        self._image_cache = None
        return super().load_state_dict(state_dict, strict=strict)

    def _apply(self, fn, *a, **k):
        self._image_cache = None
        return super()._apply(fn, *a, **k)

    def train(self, mode=True):
        if mode:
            what = "decoder_layerdrop=%r in training" % self.cfg.decoder_layerdrop if self.cfg.decoder_layerdrop else "train()"
            raise NotImplementedError("%s: training mode is not built for Wav2Vec2Seq2Seq (inference only; the decoder has no "
                                      "backward)" % what)
        return super().train(False)

    def max_decoder_positions(self):
        return self.cfg.max_target_positions

    # -- derived weight images -------------------------------------------------------------------------------------------
    def _images(self):
        """packed q|k|v of the self-attention, stacked k|v of the encoder attention, the scaled input table; built once per
        (device, dtype)"""
        d = self.decoder
        p0 = d.output_weight()
        key = (p0.device, p0.dtype)
        if self._image_cache is not None and self._image_cache[0] == key:
            return self._image_cache[1]
        im = {}
        with torch.no_grad():
            for i, l in enumerate(d.layers):
                a, e = l.self_attn, l.encoder_attn
                im["qkv_w%d" % i] = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]).contiguous()
                im["qkv_b%d" % i] = torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]).contiguous()
                im["kv_w%d" % i] = torch.cat([e.k_proj.weight, e.v_proj.weight]).contiguous()
                im["kv_b%d" % i] = torch.cat([e.k_proj.bias, e.v_proj.bias]).contiguous()
            im["embed"] = (d.embed_tokens.weight.float() * self.embed_scale).to(p0.dtype).contiguous()
        self._image_cache = (key, im)
        return im

    def _positions(self, im, T):
        cfg, d = self.cfg, self.decoder
        if cfg.no_token_positional_embeddings:
            return None
        if cfg.decoder_learned_pos:
            return d.embed_positions.weight
        need = self.pad + 1 + T
        if im.get("pos_n", 0) < need:
            p0 = d.output_weight()
            n = max(need, 2 * im.get("pos_n", 0), self.pad + 1 + 64)
            im["pos"] = sinusoidal_table(n, cfg.decoder_embed_dim, self.pad).to(device=p0.device, dtype=p0.dtype).contiguous()
            im["pos_n"] = n
        return im["pos"]

    # -- the network -----------------------------------------------------------------------------------------------------
    def _refuse_grad(self, *tensors):
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
            raise NotImplementedError("an input requires gradients: Wav2Vec2Seq2Seq is inference only (training is not built)")

    def _encode(self, source, padding_mask):
        """-> (encoder output [B, Ts, D], src_lengths int32 [B] on the device or None, K | V [B, Ts, 2 D] per layer)"""
        x, pm = self.encoder(source, padding_mask)
        return self.attend_to(x, pm)

    def attend_to(self, x, padding_mask=None):
        """encoder output x [B, Ts, D] (after proj) and its frame mask -> what the decoder needs of it: (x, src_lengths int32 [B] on
        the device or None, K | V [B, Ts, 2 D] per layer -- one wavlm_gemm against the stacked k_proj / v_proj each)"""
        from . import ops
        im, D = self._images(), self.cfg.decoder_embed_dim
        B, Ts, _ = x.shape
        x = x.reshape(B * Ts, D).contiguous()
        src_lengths = None if padding_mask is None else (~padding_mask).sum(-1).to(torch.int32).contiguous()
        kv = []
        for i in range(self.cfg.decoder_layers):
            y = torch.empty((B * Ts, 2 * D), dtype=x.dtype, device=x.device)
            ops.gemm(x, im["kv_w%d" % i], y, B * Ts, 2 * D, D, lda=D, ldb=D, ldc=2 * D, bias=im["kv_b%d" % i])
            kv.append(y.view(B, Ts, 2 * D))
        return x.view(B, Ts, D), src_lengths, kv

    def _stack(self, flat, pidx, T, self_attention, cross_attention):
        """the decoder over M rows that meet only in self_attention(layer, qkv [M, 3 D]) -> [M, D] and cross_attention(layer,
        q [M, D]) -> [M, D]: flat int32 [M] the tokens, pidx int32 [M] their rows of the position table, which covers T tokens
        -> the features [M, D] (extract_features, wav2vec2_asr.py:550-613; layers: modules/transformer_layer.py:282-403)"""
        from . import ops
        cfg, d, im = self.cfg, self.decoder, self._images()
        M, D, F = flat.numel(), cfg.decoder_embed_dim, cfg.decoder_ffn_embed_dim
        dev, dtype = flat.device, d.output_weight().dtype
        new = lambda *shape: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731

        def linear(x, w, b, K, N, res=None):
            y = new(M, N)
            ops.gemm(x, w, y, M, N, K, lda=K, ldb=K, ldc=N, bias=b, res=res, ld_res=N if res is not None else 0)
            return y

        def ln(x, r, mod):
            return ops.layernorm_fwd(x, r, mod.weight, mod.bias, mod.eps, save=False)[0]

        x = ops.gather_rows(im["embed"], flat, M)
        pos = self._positions(im, T)
        if pos is not None:
            ops.axpby_(x, ops.gather_rows(pos, pidx, M), 1.0, 1.0)
        pre = cfg.decoder_normalize_before
        for i, l in enumerate(d.layers):
            a, e = l.self_attn, l.encoder_attn
            h = ln(x, None, l.self_attn_layer_norm) if pre else x
            o = self_attention(i, linear(h, im["qkv_w%d" % i], im["qkv_b%d" % i], D, 3 * D))
            if pre:
                x = linear(o, a.out_proj.weight, a.out_proj.bias, D, D, res=x)
                h = ln(x, None, l.encoder_attn_layer_norm)
            else:
                x = ln(x, linear(o, a.out_proj.weight, a.out_proj.bias, D, D), l.self_attn_layer_norm)
                h = x
            o = cross_attention(i, linear(h, e.q_proj.weight, e.q_proj.bias, D, D))
            if pre:
                x = linear(o, e.out_proj.weight, e.out_proj.bias, D, D, res=x)
                h = ln(x, None, l.final_layer_norm)
            else:
                x = ln(x, linear(o, e.out_proj.weight, e.out_proj.bias, D, D), l.encoder_attn_layer_norm)
                h = x
            f = ops.act_fwd(linear(h, l.fc1.weight, l.fc1.bias, D, F), "relu")
            if pre:
                x = linear(f, l.fc2.weight, l.fc2.bias, F, D, res=x)
            else:
                x = ln(x, linear(f, l.fc2.weight, l.fc2.bias, F, D), l.final_layer_norm)
        if hasattr(d, "layer_norm"):
            x = ln(x, None, d.layer_norm)
        return x

    def _logits(self, x):
        """the output layer: x [M, D] -> fp32 logits [M, V] (a view of rows padded to a multiple of 4 entries)"""
        from . import ops
        w = self.decoder.output_weight()
        M, V = x.shape[0], self.vocab
        ld = (V + 3) // 4 * 4
        logits = torch.empty((M, ld), dtype=torch.float32, device=x.device)
        ops.gemm(x, w, logits, M, V, x.shape[1], lda=x.stride(0), ldb=w.stride(0), ldc=ld)
        return logits[:, :V]

    def _check_tokens(self, tokens):
        if tokens.numel() and not (0 <= int(tokens.min()) and int(tokens.max()) < self.vocab):
            raise ValueError("a token is not one of the %d dictionary entries" % self.vocab)
        if self.cfg.decoder_learned_pos and not self.cfg.no_token_positional_embeddings and \
                tokens.shape[1] > self.cfg.max_target_positions:
            raise ValueError("%d target positions are more than max_target_positions = %d of the learned positions"
                             % (tokens.shape[1], self.cfg.max_target_positions))

    def decode_forced(self, enc, prev_output_tokens):
        """enc: what _encode returned; prev_output_tokens [B, T] -> logits fp32 [B, T, V]"""
        from . import ops
        _, src_lengths, kv = enc
        tok = prev_output_tokens.to(torch.long)
        self._check_tokens(tok)
        B, T = tok.shape
        dev = kv[0].device
        H = self.cfg.decoder_attention_heads
        tok = tok.to(dev)
        keep = tok != self.pad                                    # utils.make_positions
        pidx = (torch.cumsum(keep, 1) * keep + self.pad).to(torch.int32).reshape(-1).contiguous()
        offsets = (torch.arange(B + 1, dtype=torch.int32, device=dev) * T).contiguous()
        x = self._stack(tok.to(torch.int32).reshape(-1).contiguous(), pidx, T,
                        lambda i, qkv: ops.attn_causal_fwd(qkv.view(B, T, -1), H).view(B * T, -1),
                        lambda i, q: ops.attn_cross_fwd(q, kv[i], H, offsets, src_lengths, max_group=T))
        return self._logits(x).reshape(B, T, self.vocab)

    def forward(self, source, padding_mask, prev_output_tokens):
        self._refuse_grad(source)
        with torch.no_grad():
            return self.decode_forced(self._encode(source, padding_mask), prev_output_tokens)

    # -- the search ------------------------------------------------------------------------------------------------------
    def _max_len(self, src_len, max_len_a, max_len_b):
        return min(int(max_len_a * src_len + max_len_b), self.max_decoder_positions() - 1)     # sequence_generator.py:240-250

    def _search_limits(self, B, src_len, beam, max_len_a, max_len_b, min_len):
        from . import ops
        max_len = self._max_len(src_len, max_len_a, max_len_b)
        if not 0 <= min_len <= max_len:
            raise ValueError("min_len cannot be larger than max_len (%d, %d)" % (min_len, max_len))
        if not ops.beam_step_supported(beam, self.vocab, B, torch.float32):
            raise NotImplementedError("wavlm_beam_step takes 1 <= beam <= 32, 2 <= V <= 65536, B <= 65535 (beam=%d V=%d B=%d)"
                                      % (beam, self.vocab, B))
        return max_len

    def generate(self, source, padding_mask=None, beam=5, max_len_a=0, max_len_b=200, min_len=1, normalize_scores=True,
                 len_penalty=1.0, unk_penalty=0.0, temperature=1.0, nbest=None, step_logits=None, **refused):
        """-> per sentence its finished hypotheses, best first (at most `nbest`; default all `beam`), each {"tokens": long [n]
        ending in eos, "score": fp32 scalar, "positional_scores": fp32 [n]} as SequenceGenerator returns them.
        step_logits (tests): a list that receives every step's fp32 logits [B * beam, V] and row lengths."""
        for k, v in refused.items():
            if k in GENERATE_REFUSED:
                if v is not None and v is not False and not (isinstance(v, (int, float)) and v == 0):
                    if k in FUSION_OPTIONS:
                        raise NotImplementedError("%s is not an option of generate: unispeech_amd.sequence_generator."
                                                  "SequenceGenerator takes it" % k)
                    raise NotImplementedError("%s is not built (see unispeech_amd/seq2seq.py)" % k)
            else:
                raise TypeError("generate: unknown option %r" % k)
        self._refuse_grad(source)
        max_len = self._search_limits(source.shape[0], source.shape[1], beam, max_len_a, max_len_b, min_len)   # before the encoder
        with torch.no_grad():
            enc = self._encode(source, padding_mask)
        return self._search(enc, max_len, beam, min_len, normalize_scores, len_penalty, unk_penalty, temperature, nbest,
                            step_logits)

    def search(self, enc, src_len, beam=5, max_len_a=0, max_len_b=200, min_len=1, normalize_scores=True, len_penalty=1.0,
               unk_penalty=0.0, temperature=1.0, nbest=None, step_logits=None, *, max_len=None, lm_model=None, lm_weight=1.0,
               no_repeat_ngram_size=0):
        """generate() behind the encoder: enc is what attend_to returned, src_len the padded source length max_len is taken from
        (max_len: an upper limit of its own on top, SequenceGenerator's).  lm_model (a TransformerLM over the same dictionary),
        lm_weight: shallow fusion; no_repeat_ngram_size: the n-gram blocker (unispeech_amd/sequence_generator.py is the public
        entry to both)."""
        limit = self._search_limits(enc[0].shape[0], src_len, beam, max_len_a, max_len_b, min_len)
        if max_len is not None:
            limit = min(limit, int(max_len))
            if min_len > limit:
                raise ValueError("min_len cannot be larger than max_len (%d, %d)" % (min_len, limit))
        self._check_fusion(lm_model, lm_weight, no_repeat_ngram_size, limit, enc[2][0].device)
        return self._search(enc, limit, beam, min_len, normalize_scores, len_penalty, unk_penalty, temperature, nbest,
                            step_logits, lm_model=lm_model, lm_weight=lm_weight, no_repeat_ngram_size=no_repeat_ngram_size)

    def _check_fusion(self, lm_model, lm_weight, no_repeat_ngram_size, max_len, device):
        """what the fused search refuses, before anything runs"""
        from .transformer_lm import TransformerLM
        if int(no_repeat_ngram_size) < 0:
            raise ValueError("no_repeat_ngram_size must be >= 0, got %r" % (no_repeat_ngram_size,))
        if lm_model is None:
            return
        if not isinstance(lm_model, TransformerLM):
            raise NotImplementedError("lm_model must be a unispeech_amd.transformer_lm.TransformerLM, got %s"
                                      % type(lm_model).__name__)
        if not math.isfinite(float(lm_weight)):
            raise ValueError("lm_weight must be finite, got %r" % (lm_weight,))
        mine, theirs = (self.vocab, self.pad, self.eos, self.unk), (lm_model.vocab, lm_model.pad, lm_model.eos, lm_model.unk)
        if mine != theirs:
            raise ValueError("lm_model's dictionary (vocab, pad, eos, unk) = %r differs from the model's %r" % (theirs, mine))
        lm_dev = lm_model.decoder.output_projection.weight.device
        if lm_dev != torch.device(device):
            raise ValueError("lm_model is on %s, the model on %s" % (lm_dev, device))
        lc = lm_model.cfg
        if lc.decoder_learned_pos and not lc.no_token_positional_embeddings and max_len + 1 > lc.max_target_positions:
            raise ValueError("max_len + 1 = %d target positions are more than max_target_positions = %d of lm_model's learned "
                             "positions" % (max_len + 1, lc.max_target_positions))
        hd = lc.decoder_embed_dim // lc.decoder_attention_heads
        if hd * lc.decoder_attention_heads != lc.decoder_embed_dim or hd not in (32, 64):
            raise NotImplementedError("lm_model: wavlm_attn_step takes heads 32 or 64 wide, not %d / %d"
                                      % (lc.decoder_embed_dim, lc.decoder_attention_heads))

    def _search(self, enc, max_len, beam, min_len, normalize_scores, len_penalty, unk_penalty, temperature, nbest, step_logits,
                *, lm_model=None, lm_weight=1.0, no_repeat_ngram_size=0):
        from . import ops
        B, V = enc[0].shape[0], self.vocab
        cfg = self.cfg
        H, D, L = cfg.decoder_attention_heads, cfg.decoder_embed_dim, cfg.decoder_layers
        fused = lm_model is not None or int(no_repeat_ngram_size) > 0
        with torch.no_grad():
            _, src_lengths, kv = enc
            dev, dtype = kv[0].device, kv[0].dtype
            R = B * beam
            st = ops.BeamState(B, beam, max_len, self.eos, dev)
            slots = (max_len + 1) * R
            kc = [torch.zeros((slots, D), dtype=dtype, device=dev) for _ in range(L)]
            vc = [torch.zeros((slots, D), dtype=dtype, device=dev) for _ in range(L)]
            offsets = (torch.arange(B + 1, dtype=torch.int32, device=dev) * beam).contiguous()
            self._positions(self._images(), max_len + 1)
            if lm_model is not None:                                  # the LM's own caches over the same tree of slots
                lc = lm_model.cfg
                H_lm, lm_w = lc.decoder_attention_heads, lm_model.decoder.output_projection.weight
                lm_kc = [torch.zeros((slots, lc.decoder_embed_dim), dtype=lm_w.dtype, device=dev) for _ in range(lc.decoder_layers)]
                lm_vc = [torch.zeros((slots, lc.decoder_embed_dim), dtype=lm_w.dtype, device=dev) for _ in range(lc.decoder_layers)]
                lm_model._positions(lm_model._images(), max_len + 1)
            self.loop_reads = self.loop_steps = 0
            for step in range(max_len + 1):
                self.loop_steps = step + 1
                lengths, anc = st.lengths, st.anc[step % 2]
                pidx = (lengths + self.pad).contiguous()              # position row pad + 1 + step; a dead row: the pad row
                x = self._stack(st.tokens, pidx, step + 1,
                                lambda i, qkv: ops.attn_step(qkv, kc[i], vc[i], st.slots, anc, lengths, H, step + 1),
                                lambda i, q: ops.attn_cross_fwd(q, kv[i], H, offsets, src_lengths, live=lengths, max_group=beam))
                logits = self._logits(x)
                if fused:
                    lm_logits = None
                    if lm_model is not None:                          # a plain log-softmax scores it: no unk rule here
                        y = lm_model._stack(st.tokens, pidx, step + 1,
                                            lambda i, qkv: ops.attn_step(qkv, lm_kc[i], lm_vc[i], st.slots, anc, lengths, H_lm,
                                                                         step + 1))
                        ld = (V + 3) // 4 * 4
                        lm_logits = torch.empty((R, ld), dtype=torch.float32, device=dev)
                        ops.gemm(y, lm_w, lm_logits, R, V, y.shape[1], lda=y.stride(0), ldb=lm_w.stride(0), ldc=ld)
                        lm_logits = lm_logits[:, :V]
                    if step_logits is not None:
                        step_logits.append((logits.clone(), lengths.clone(), None if lm_logits is None else lm_logits.clone()))
                    ops.beam_step_fused(logits, st, V, max_len=max_len, min_len=min_len, pad=self.pad, unk=self.unk, eos=self.eos,
                                        lm_logits=lm_logits, lm_weight=lm_weight, no_repeat_ngram_size=no_repeat_ngram_size,
                                        unk_penalty=unk_penalty, temperature=temperature, len_penalty=len_penalty,
                                        normalize_scores=normalize_scores, step=step)
                else:
                    if step_logits is not None:
                        step_logits.append((logits.clone(), lengths.clone()))
                    ops.beam_step(logits, st, V, max_len=max_len, min_len=min_len, pad=self.pad, unk=self.unk, eos=self.eos,
                                  unk_penalty=unk_penalty, temperature=temperature, len_penalty=len_penalty,
                                  normalize_scores=normalize_scores, step=step)
                if step % READ_EVERY == READ_EVERY - 1 and step < max_len:
                    self.loop_reads += 1
                    if int(read_device(st.finished)) >= B:
                        break
            return _collect(st.n_fin.cpu(), st.fin_f.cpu(), st.fin_i.cpu(), st.tree_parent.cpu(), st.tree_token.cpu(),
                            st.tree_score.cpu(), self.eos, beam if nbest is None else nbest)


def _collect(n_fin, fin_f, fin_i, tree_parent, tree_token, tree_score, eos, nbest):
    """the finished lists and the tree, read once -> hypotheses, sorted by score (stable, as sequence_generator.py:551-557)"""
    out = []
    for b in range(n_fin.numel()):
        hyps = []
        for j in range(int(n_fin[b])):
            toks, pos = [eos], [float(fin_f[b, j, 2])]
            s = int(fin_i[b, j, 0])
            while int(tree_parent[s]) >= 0:                           # the slots of step 0 hold the bos and have no parent
                toks.append(int(tree_token[s]))
                pos.append(float(tree_score[s]))
                s = int(tree_parent[s])
            assert len(toks) == int(fin_i[b, j, 1])
            hyps.append({"tokens": torch.tensor(toks[::-1], dtype=torch.long), "score": fin_f[b, j, 0].clone(),
                         "positional_scores": torch.tensor(pos[::-1], dtype=torch.float32)})
        order = sorted(range(len(hyps)), key=lambda i: -float(hyps[i]["score"]))
        out.append([hyps[i] for i in order][:nbest])
    return out


# --------------------------------------------------------------------------------------------------- float64 reference
def encoder_proj_reference(model, x):
    """encoder features [B, Ts, d] -> what the decoder attends to, float64 (Wav2VecEncoder.forward's proj)"""
    x = x.double()
    return _lin64(x, model.encoder.proj) if model.encoder.proj is not None else x


def decoder_reference(model, encoder_out, padding_mask, tokens):
    """the decoder in float64 on the CPU, one sentence at a time (nothing depends on the batch): encoder_out [B, Ts, D] (after
    proj), padding_mask bool [B, Ts] or None, tokens long [B, T] (right-padded with pad, which the reference attends like any
    token) -> logits float64 [B, T, V]"""
    cfg, d = model.cfg, model.decoder
    D, H = cfg.decoder_embed_dim, cfg.decoder_attention_heads
    hd = D // H
    pre = cfg.decoder_normalize_before
    tokens = tokens.to(torch.long)
    B, T = tokens.shape
    out = []
    with torch.no_grad():
        future = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
        for b in range(B):
            tok = tokens[b]
            n = encoder_out.shape[1] if padding_mask is None else int((~padding_mask[b]).sum())
            enc = encoder_out[b, :n].double()
            x = model.embed_scale * d.embed_tokens.weight.double()[tok]
            if not cfg.no_token_positional_embeddings:
                keep = tok != model.pad
                idx = torch.cumsum(keep, 0) * keep + model.pad
                tab = d.embed_positions.weight if cfg.decoder_learned_pos else sinusoidal_table(model.pad + 1 + T, D, model.pad)
                x = x + tab.double()[idx]
            for l in d.layers:
                a, e = l.self_attn, l.encoder_attn
                h = _ln64(x, l.self_attn_layer_norm) if pre else x
                o = _attend64(_lin64(h, a.q_proj) * hd ** -0.5, _lin64(h, a.k_proj), _lin64(h, a.v_proj), H, future)
                x = x + _lin64(o, a.out_proj)
                if not pre:
                    x = _ln64(x, l.self_attn_layer_norm)
                h = _ln64(x, l.encoder_attn_layer_norm) if pre else x
                o = _attend64(_lin64(h, e.q_proj) * hd ** -0.5, _lin64(enc, e.k_proj), _lin64(enc, e.v_proj), H)
                x = x + _lin64(o, e.out_proj)
                if not pre:
                    x = _ln64(x, l.encoder_attn_layer_norm)
                h = _ln64(x, l.final_layer_norm) if pre else x
                x = x + _lin64(torch.relu(_lin64(h, l.fc1)), l.fc2)
                if not pre:
                    x = _ln64(x, l.final_layer_norm)
            if hasattr(d, "layer_norm"):
                x = _ln64(x, d.layer_norm)
            out.append(x @ d.output_weight().double().t())
    return torch.stack(out)


def beam_step_reference(logits, cum, step, n_fin, *, beam, max_len, min_len, pad, unk, eos, unk_penalty=0.0, temperature=1.0,
                        len_penalty=1.0, normalize_scores=True, full=False, lm_logits=None, lm_weight=1.0, history=None,
                        no_repeat_ngram_size=0):
    """one sentence, one step, float64: logits [n_live, V] of its live rows, cum [n_live] their cumulative scores, n_fin the
    entries its finished list holds -> {"candidates": [(score, k * V + token)] in order, "finished": [(score, raw score, step
    score, parent row k, length)], "rows": [(parent row k, token, cumulative score, step score)], "done": bool}.  The rules of
    sequence_generator.py:346-367 and 405-520 with search.py:119-136; ties go to the smaller k * V + token.
    lm_logits [n_live, V]: lm_weight * log_softmax(lm_logits) is added before the NaN rule (338-346; 0 * -inf is NaN, hence
    -inf).  no_repeat_ngram_size = n > 0 with history (per row its tokens h[0 .. step], h[0] the bos): after the other rules every
    token that would repeat an n-gram of h is -inf (ngram_repeat_block.py:96-143, n = 1 included: every token of h);
    "banned": the rows' sets of such tokens."""
    x = torch.as_tensor(logits, dtype=torch.float64) / temperature
    cum = torch.as_tensor(cum, dtype=torch.float64)
    n, V = x.shape
    lp = torch.log_softmax(x, -1)
    if lm_logits is not None:
        lp = lp + lm_weight * torch.log_softmax(torch.as_tensor(lm_logits, dtype=torch.float64), -1)
    lp[lp != lp] = -math.inf
    lp[:, pad] = -math.inf
    lp[:, unk] -= unk_penalty
    if step >= max_len:
        lp[:, :eos] = -math.inf
        lp[:, eos + 1:] = -math.inf
    if step < min_len:
        lp[:, eos] = -math.inf
    banned = None
    if no_repeat_ngram_size > 0:
        if history is None or len(history) != n:
            raise ValueError("no_repeat_ngram_size needs the history of each of the %d rows" % n)
        banned = [ngram_banned(h, step, no_repeat_ngram_size) for h in history]
        for k, ban in enumerate(banned):
            for t in ban:
                if 0 <= t < V:
                    lp[k, t] = -math.inf
    sc = (lp + cum.unsqueeze(1)).reshape(-1)
    sc[sc != sc] = -math.inf
    K2 = min(2 * beam, n * V - 1)
    vals = sc.numpy()
    order = np.lexsort((np.arange(vals.size), -vals))[:K2]            # score descending, then flat index ascending
    cands = [(float(vals[i]), int(i)) for i in order]
    finished, rows = [], []
    for c, (s, i) in enumerate(cands):
        k, tok = divmod(i, V)
        if tok == eos and s > -math.inf:
            if c < beam and n_fin + len(finished) < beam:
                finished.append((s / (step + 1) ** len_penalty if normalize_scores else s, s, s - float(cum[k]), k, step + 1))
        elif len(rows) < beam:
            rows.append((k, tok, s, s - float(cum[k])))
    done = n_fin + len(finished) >= beam or step >= max_len or not rows
    res = {"candidates": cands, "finished": finished, "rows": [] if done else rows, "done": done}
    if banned is not None:
        res["banned"] = banned
    if full:                                                          # every entry in order, and the rows before `done` cut them
        res["all"] = [(float(vals[i]), int(i)) for i in np.lexsort((np.arange(vals.size), -vals))]
        res["rows_taken"] = rows
    return res


def ngram_banned(h, step, n):
    """the tokens _no_repeat_ngram bans after the history h[0 .. step] (h[0] the bos): for every i in 0 .. step + 1 - n with
    h[i .. i + n - 2] == h[step + 2 - n .. step], token h[i + n - 1].  The reference builds its n-grams over the whole padded
    row; the further ones can only ban pad, which is -inf already."""
    h = [int(t) for t in h]
    if len(h) != step + 1:
        raise ValueError("a history of %d tokens at step %d" % (len(h), step))
    cnt = step + 2 - n
    tail = h[cnt:] if cnt >= 0 else None
    return {h[i + n - 1] for i in range(max(cnt, 0)) if h[i:i + n - 1] == tail}


def beam_search_reference(step_logits_fn, B, *, bos, beam=5, max_len=200, min_len=1, pad=1, unk=3, eos=2, unk_penalty=0.0,
                          temperature=1.0, len_penalty=1.0, normalize_scores=True, nbest=None, margins=None, lm_logits_fn=None,
                          lm_weight=1.0, no_repeat_ngram_size=0):
    """SequenceGenerator._generate + BeamSearch.step + finalize_hypos restated in float64 on the host.
    step_logits_fn(b, prefixes) -> logits [len(prefixes), V] of the next token after each prefix (lists of ids that begin with
    bos) of sentence b.  -> per sentence the finished hypotheses sorted by score, each {"tokens", "score", "positional_scores"}.
    margins (a list): receives, per sentence and step, the gap between the last candidate taken and the first one left out.
    lm_logits_fn(b, prefixes) -> the LM's logits [len(prefixes), V] (None: no LM), weighed by lm_weight; no_repeat_ngram_size:
    the blocker over the prefixes."""
    opts = dict(beam=beam, max_len=max_len, min_len=min_len, pad=pad, unk=unk, eos=eos, unk_penalty=unk_penalty,
                temperature=temperature, len_penalty=len_penalty, normalize_scores=normalize_scores)
    out = []
    for b in range(B):
        prefixes, cum, pos, hyps = [[bos]], [0.0], [[]], []
        for step in range(max_len + 1):
            logits = torch.as_tensor(step_logits_fn(b, prefixes), dtype=torch.float64)
            extra = {}
            if lm_logits_fn is not None:
                extra.update(lm_logits=torch.as_tensor(lm_logits_fn(b, prefixes), dtype=torch.float64), lm_weight=lm_weight)
            if no_repeat_ngram_size > 0:
                extra.update(history=prefixes, no_repeat_ngram_size=no_repeat_ngram_size)
            r = beam_step_reference(logits, cum, step, len(hyps), **opts, **extra)
            if margins is not None:
                margins.append(_margin(logits, cum, step, r, dict(opts, **extra)))
            for score, raw, ss, k, length in r["finished"]:
                hyps.append({"tokens": torch.tensor(prefixes[k][1:] + [eos], dtype=torch.long),
                             "score": torch.tensor(score, dtype=torch.float64),
                             "positional_scores": torch.tensor(pos[k] + [ss], dtype=torch.float64)})
            if r["done"]:
                break
            prefixes, cum, pos = ([prefixes[k] + [tok] for k, tok, _, _ in r["rows"]], [s for _, _, s, _ in r["rows"]],
                                  [pos[k] + [ss] for k, _, _, ss in r["rows"]])
        order = sorted(range(len(hyps)), key=lambda i: -float(hyps[i]["score"]))
        out.append([hyps[i] for i in order][:beam if nbest is None else nbest])
    return out


def _margin(logits, cum, step, r, opts):
    """the smallest float64 gap that decides this step: between the worst candidate taken as a row and the best non-eos one that
    was not, and between every finite eos candidate and the rank `beam` it must be above to be finalized (or is below)"""
    V, eos, beam = logits.shape[1], opts["eos"], opts["beam"]
    f = beam_step_reference(logits, cum, step, 0, full=True, **opts)
    ranked = f["all"]
    is_eos = [i % V == eos and s > -math.inf for s, i in ranked]
    gaps = []
    others = [s for (s, _), e in zip(ranked, is_eos) if not e]
    if len(others) > beam and others[beam - 1] > -math.inf:
        gaps.append(others[beam - 1] - others[beam])
    for c, ((s, _), e) in enumerate(zip(ranked, is_eos)):
        if e and len(ranked) > beam:
            gaps.append(s - ranked[beam][0] if c < beam else ranked[beam - 1][0] - s)
    return min(gaps) if gaps else math.inf


def generate_reference(model, encoder_out, padding_mask, src_len, beam=5, max_len_a=0, max_len_b=200, min_len=1, lm_model=None,
                       **kw):
    """Wav2Vec2Seq2Seq.generate's result in float64 on the CPU from the encoder's output [B, Ts, D] (after proj): every step
    re-runs decoder_reference over the whole prefix -- and, with lm_model (a TransformerLM; lm_weight=, and
    no_repeat_ngram_size= likewise), transformer_lm._forward64 over it"""
    max_len = model._max_len(src_len, max_len_a, max_len_b)
    if lm_model is not None:
        from .transformer_lm import _forward64

        def lm_fn(b, prefixes):
            with torch.no_grad():
                return torch.stack([_forward64(lm_model, p[1:])[-1] for p in prefixes])
        kw["lm_logits_fn"] = lm_fn

    def fn(b, prefixes):
        tok = torch.tensor(prefixes, dtype=torch.long)
        pm = None if padding_mask is None else padding_mask[b:b + 1].expand(len(prefixes), -1)
        return decoder_reference(model, encoder_out[b:b + 1].expand(len(prefixes), -1, -1), pm, tok)[:, -1]
    return beam_search_reference(fn, encoder_out.shape[0], bos=model.eos, beam=beam, max_len=max_len, min_len=min_len,
                                 pad=model.pad, unk=model.unk, eos=model.eos, **kw)


# --------------------------------------------------------------------------------------------------------- command line
def parse_args(argv=None):
    from .ctc import base_parser
    p, d, c = base_parser("python -m unispeech_amd.seq2seq", __doc__.split("\n\n")[0],
                          decode_help="beam-search transcripts, one line per file (with --nbest above 1: score, then text)",
                          score_help="UER / WER of the beam search's 1-best over a manifest")
    for q in (d, c):
        q.add_argument("--beam", type=int, default=5)
        q.add_argument("--max-len-a", type=float, default=0.0)
        q.add_argument("--max-len-b", type=int, default=200)
        q.add_argument("--lenpen", type=float, default=1.0)
        q.add_argument("--nbest", type=int, default=1)
        q.add_argument("--lm", default=None, metavar="LM.pt", help="a TransformerLM checkpoint over the same DICT: shallow fusion")
        q.add_argument("--lm-weight", type=float, default=1.0)
        q.add_argument("--no-repeat-ngram-size", type=int, default=0, metavar="N", help="no n-gram occurs twice in a hypothesis")
    return p.parse_args(argv)


def _load(a):
    from .ctc import LetterDictionary
    d = LetterDictionary.load(a.dict)
    model = Wav2Vec2Seq2Seq.from_checkpoint(a.ckpt, d).cuda()
    if a.bf16:
        model = model.to(torch.bfloat16)
    return d, model, next(model.parameters()).dtype


def _search_kwargs(a):
    return dict(beam=a.beam, max_len_a=a.max_len_a, max_len_b=a.max_len_b, len_penalty=a.lenpen, nbest=a.nbest)


def _generator(a, d, model, nbest=None):
    """source, padding_mask -> hypotheses: generate() itself, or SequenceGenerator where an LM or the blocker is asked for"""
    kw = dict(_search_kwargs(a), nbest=a.nbest if nbest is None else nbest)
    if a.lm is None and not a.no_repeat_ngram_size:
        return lambda src, pm: model.generate(src, pm, **kw)
    from .sequence_generator import SequenceGenerator
    from .transformer_lm import TransformerLM
    lm = None
    if a.lm is not None:
        lm = TransformerLM.from_checkpoint(a.lm, len(d), pad=d.pad(), eos=d.eos(), unk=d.unk()).cuda()
        lm = lm.to(next(model.parameters()).dtype)
    gen = SequenceGenerator([model], d, beam_size=a.beam, max_len_a=a.max_len_a, max_len_b=a.max_len_b, len_penalty=a.lenpen,
                            no_repeat_ngram_size=a.no_repeat_ngram_size, lm_model=lm, lm_weight=a.lm_weight)
    return lambda src, pm: [h[:kw["nbest"]] for h in gen.generate([model], {"net_input": {"source": src, "padding_mask": pm}})]


def _strip(tokens, d):
    return [int(t) for t in tokens if int(t) not in (d.pad(), d.eos())]


def decode(a):
    from .ctc import post_process
    from .kmeans import read_wav
    d, model, dtype = _load(a)
    run = _generator(a, d, model)
    symbol = None if a.post_process == "none" else "letter"
    for path in a.wavs:
        wav, sr = read_wav(path)
        if sr != 16000:
            raise NotImplementedError("%s: %d Hz; the models take 16 kHz audio (unispeech_amd.resample converts)" % (path, sr))
        x = torch.as_tensor(wav, dtype=torch.float32).cuda()
        if getattr(model, "normalize", False):
            x = torch.nn.functional.layer_norm(x, x.shape)
        for h in run(x.view(1, -1).to(dtype), None)[0]:
            text = post_process(d.string(_strip(h["tokens"], d)), symbol)
            print(text if a.nbest == 1 else "%.4f\t%s" % (float(h["score"]), text))
    return 0


def score(a):
    """`score`: ctc.score's manifest batching, host edit distances and result files around the beam search's 1-best"""
    from .ctc import edit_distance, length_batches, post_process, read_labels, read_manifest
    from .kmeans import read_wav
    d, model, dtype = _load(a)
    run = _generator(a, d, model, nbest=1)
    symbol = None if a.post_process == "none" else "letter"
    entries = read_manifest(a.manifest)
    labels = read_labels(a.labels, d, len(entries))
    total = np.zeros(4, dtype=np.int64)
    hyps = [[] for _ in entries]
    for batch in length_batches([n for _, n in entries], int(a.batch_seconds * 16000)):
        wavs = []
        for i in batch:
            wav, sr = read_wav(entries[i][0])
            if sr != 16000:
                raise NotImplementedError("%s: %d Hz; the models take 16 kHz audio (unispeech_amd.resample converts)"
                                          % (entries[i][0], sr))
            x = torch.as_tensor(wav, dtype=torch.float32)
            wavs.append(torch.nn.functional.layer_norm(x, x.shape) if getattr(model, "normalize", False) else x)
        n = max(w.numel() for w in wavs)
        src = torch.zeros(len(batch), n)
        pm = torch.ones(len(batch), n, dtype=torch.bool)
        for r, w in enumerate(wavs):
            src[r, :w.numel()] = w
            pm[r, :w.numel()] = False
        res = run(src.cuda().to(dtype), pm.cuda() if bool(pm.any()) else None)
        for r, i in enumerate(batch):
            pred = _strip(res[r][0]["tokens"], d) if res[r] else []
            targ = [v for v in labels[i] if v not in (d.pad(), d.eos())]
            pw, tw = post_process(d.string(pred), symbol).split(), post_process(d.string(targ), symbol).split()
            total += np.array([edit_distance(pred, targ), len(targ), edit_distance(pw, tw), len(tw)], dtype=np.int64)
            hyps[i] = pred
    c_err, c_len, w_err, w_len = (int(v) for v in total)
    print("UER %.3f%% WER %.3f%% c_errors %d c_total %d w_errors %d w_total %d"
          % (c_err * 100.0 / max(c_len, 1), w_err * 100.0 / max(w_len, 1), c_err, c_len, w_err, w_len))
    if a.results is not None:
        os.makedirs(a.results, exist_ok=True)
        files = {"hypo.units": [], "hypo.word": [], "ref.units": [], "ref.word": []}
        for i, (hyp, ref) in enumerate(zip(hyps, labels)):            # infer.py:120-148, speaker None, id = the utterance's index
            for kind, toks in (("hypo", hyp), ("ref", ref)):
                units = d.string(toks)
                files[kind + ".units"].append("%s (None-%d)" % (units, i))
                files[kind + ".word"].append("%s (None-%d)" % (post_process(units, symbol), i))
        for name, lines in files.items():
            with open(os.path.join(a.results, name), "w", encoding="utf-8") as f:
                f.write("".join(line + "\n" for line in lines))
    return 0


def main(argv=None):
    a = parse_args(argv)
    return score(a) if a.cmd == "score" else decode(a)


if __name__ == "__main__":
    sys.exit(main())
