"""Transformer language model on the device, for second-pass rescoring (csrc/lm.hip, additive to ABI 30): the inference path
of the reference's `TransformerLanguageModel` (src/fairseq/models/transformer_lm.py, a decoder-only `TransformerDecoder` of
models/transformer.py) scored the way `FairseqLM` of examples/speech_recognition/w2l_decoder.py scores it.

  TransformerLM     parameter and buffer names equal the reference's, so `load_state_dict` takes its state dict as it stands
                    (`decoder.embed_tokens...`, `decoder.layers.N.self_attn.{q,k,v,out}_proj`, `decoder.output_projection.weight`,
                    AdaptiveInput's `embeddings.i.{0,1}.weight`, ...).  Honoured: pre-LN and post-LN, no_decoder_final_norm, relu
                    and gelu, sinusoidal and learned positions, no_token_positional_embeddings, no_scale_embedding,
                    layernorm_embedding, share_decoder_input_output_embed, adaptive_input with cut-offs and factor,
                    decoder_input_dim / decoder_output_dim other than decoder_embed_dim.  The reference's decoder never builds an
                    adaptive softmax (`self.adaptive_softmax = None`, transformer.py:737): the output is one bias-free Linear.
                    Refused by name: character_embeddings, base_layers, cross_self_attention, tie_adaptive_weights, a head width
                    other than 32 or 64.  Quant-noise is a no-op at inference and its options are ignored.
  score(sentences)  lists of word ids -> (token log-probs [N, Tmax], totals [N]), natural log, FairseqLM's conventions: input
                    [eos, w_1 .. w_n], targets [w_1 .. w_n, eos]; an `unk` target scores -inf; the empty sentence scores
                    log p(eos | eos).  Sentences are sorted by length, batched right-padded in at most `max_tokens` rows, and only
                    the hidden rows that have a target reach the output layer.
  score_reference   the same rules in float64 torch on the CPU: the specification.
  incremental()     IncrementalStates: decoder states over a tree of word histories with a KV cache (csrc/lm_step.hip
                    wavlm_attn_step), a beam's worth of new states per call -- what the first pass of
                    ctc_lexicon.fused_lexicon_decode asks for.  The reference's FairseqLM has no working cache
                    (`save_incremental = False`, w2l_decoder.py:298) and re-runs the whole prefix per state.
  incremental_reference   the same interface in float64 on the CPU: the specification.
  python -m unispeech_amd.transformer_lm score LM.pt DICT.txt [FILE]

How a layer runs: wavlm_gemm (bias, GELU and residual epilogues; q|k|v packed once into a single GEMM), wavlm_act_fwd for ReLU,
wavlm_layernorm_fwd with its residual input, wavlm_gather_rows for the embeddings, wavlm_attn_causal_fwd for the attention and
wavlm_lm_logprob for the output layer: the [rows, V] logits never exist.  WAVLM_LM_LOGPROB_COMPOSED=1 (read at every call)
runs the output layer as wavlm_gemm into fp32 logits + wavlm_ce_rows in row chunks of a fixed budget instead -- what one would
do without the kernel: the fall-back for shapes it does not take and the baseline of tools/transformer_lm_bench.py.
Inference only.  bf16 and fp32 (parity) modes: `.to(torch.bfloat16)` as the other heads have it.
"""
import math
import os
import sys

import torch
import torch.nn as nn

__all__ = ["TransformerLM", "TransformerLMConfig", "score_reference", "lm_logprob", "sinusoidal_table", "IncrementalStates",
           "incremental_reference"]

COMPOSED_BUDGET_BYTES = 256 << 20      # fp32 logits of one row chunk of the composed output layer
REFUSED = ("character_embeddings", "base_layers", "cross_self_attention", "tie_adaptive_weights")


def _int_list(v):
    if v is None or v == "":
        return []
    if isinstance(v, str):
        return [int(x) for x in v.replace("[", "").replace("]", "").split(",") if x.strip()]
    return [int(x) for x in v]


class TransformerLMConfig:
    """the model options of the reference's transformer_lm (base_lm_architecture's names and defaults) from a dict, a Namespace or
    keywords; a fairseq `cfg` with a `model` group is unwrapped"""
    DEFAULTS = dict(decoder_embed_dim=512, decoder_ffn_embed_dim=2048, decoder_layers=6, decoder_attention_heads=8,
                    decoder_input_dim=None, decoder_output_dim=None, decoder_normalize_before=True, no_decoder_final_norm=False,
                    activation_fn="relu", decoder_learned_pos=False, no_token_positional_embeddings=False,
                    no_scale_embedding=False, layernorm_embedding=False, share_decoder_input_output_embed=False,
                    adaptive_input=False, adaptive_input_factor=4, adaptive_input_cutoff=None, character_embeddings=False,
                    base_layers=0, cross_self_attention=False, tie_adaptive_weights=False, max_target_positions=None,
                    tokens_per_sample=1024)

    def __init__(self, options=None, **kw):
        if options is not None and not isinstance(options, dict):
            options = dict(vars(options))
        options = dict(options or {})
        if isinstance(options.get("model"), dict) or hasattr(options.get("model"), "__dict__"):
            m = options["model"]
            options = dict(m if isinstance(m, dict) else vars(m))
        options.update(kw)
        for k, v in self.DEFAULTS.items():
            setattr(self, k, options.get(k, v))
        if self.activation_fn is None:
            self.activation_fn = "relu"
        if self.decoder_input_dim is None:
            self.decoder_input_dim = self.decoder_embed_dim
        if self.decoder_output_dim is None:
            self.decoder_output_dim = self.decoder_embed_dim
        if self.max_target_positions is None:
            self.max_target_positions = self.tokens_per_sample
        self.adaptive_input_cutoff = _int_list(self.adaptive_input_cutoff)

    def as_dict(self):
        return {k: getattr(self, k) for k in self.DEFAULTS}


def sinusoidal_table(n, dim, padding_idx):
    """the tensor2tensor table fairseq builds: [sin | cos] halves over frequencies 10000^(-i / (dim / 2 - 1)), an odd width
    zero-padded, the padding row zero; fp32 arithmetic, as the reference evaluates it"""
    half = dim // 2
    step = math.log(10000) / (half - 1)
    freq = torch.exp(torch.arange(half, dtype=torch.float32) * -step)
    ang = torch.arange(n, dtype=torch.float32).unsqueeze(1) * freq.unsqueeze(0)
    tab = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
    if dim % 2:
        tab = torch.cat([tab, torch.zeros(n, 1)], dim=1)
    tab[padding_idx] = 0
    return tab


# ------------------------------------------------------------------------------------------------ parameter containers
# (the reference's module tree: names only -- none of these modules' forward is ever called)
class _SelfAttention(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(D, D) for _ in range(4))


class _Layer(nn.Module):
    def __init__(self, D, F):
        super().__init__()
        self.self_attn = _SelfAttention(D)
        self.self_attn_layer_norm = nn.LayerNorm(D)
        self.fc1, self.fc2 = nn.Linear(D, F), nn.Linear(F, D)
        self.final_layer_norm = nn.LayerNorm(D)


class _AdaptiveInput(nn.Module):
    def __init__(self, V, pad, initial_dim, factor, output_dim, cutoff):
        super().__init__()
        cutoff = list(cutoff)
        if not cutoff or V > cutoff[-1]:
            cutoff = cutoff + [V]
        elif V != cutoff[-1]:
            raise ValueError("adaptive_input_cutoff %s goes beyond the %d dictionary entries" % (cutoff, V))
        self.cutoff = cutoff
        self.embeddings = nn.ModuleList()
        for i, c in enumerate(cutoff):
            dim = int(initial_dim // (factor ** i))
            self.embeddings.append(nn.Sequential(nn.Embedding(c - (cutoff[i - 1] if i else 0), dim),
                                                 nn.Linear(dim, output_dim, bias=False)))
        self.register_buffer("_float_tensor", torch.zeros(1))


class _Sinusoidal(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("_float_tensor", torch.zeros(1))


class _Decoder(nn.Module):
    def __init__(self, cfg, V, pad):
        super().__init__()
        D, Din, Dout = cfg.decoder_embed_dim, cfg.decoder_input_dim, cfg.decoder_output_dim
        self.register_buffer("version", torch.Tensor([3]))
        if cfg.adaptive_input:
            self.embed_tokens = _AdaptiveInput(V, pad, Din, cfg.adaptive_input_factor, D, cfg.adaptive_input_cutoff)
            Din = D
        else:
            self.embed_tokens = nn.Embedding(V, Din, pad)
        if Din != D:
            self.project_in_dim = nn.Linear(Din, D, bias=False)
        if not cfg.no_token_positional_embeddings:
            self.embed_positions = (nn.Embedding(cfg.max_target_positions + pad + 1, D, pad) if cfg.decoder_learned_pos
                                    else _Sinusoidal())
        if cfg.layernorm_embedding:
            self.layernorm_embedding = nn.LayerNorm(D)
        self.layers = nn.ModuleList([_Layer(D, cfg.decoder_ffn_embed_dim) for _ in range(cfg.decoder_layers)])
        if cfg.decoder_normalize_before and not cfg.no_decoder_final_norm:
            self.layer_norm = nn.LayerNorm(D)
        if D != Dout:
            self.project_out_dim = nn.Linear(D, Dout, bias=False)
        if cfg.share_decoder_input_output_embed:
            if cfg.adaptive_input:
                raise ValueError("share_decoder_input_output_embed needs a plain input embedding, not adaptive_input")
            if Din != Dout:
                raise ValueError("share_decoder_input_output_embed: decoder_input_dim %d is not decoder_output_dim %d" % (Din, Dout))
            self.output_projection = nn.Linear(Din, V, bias=False)
            self.output_projection.weight = self.embed_tokens.weight
        else:
            self.output_projection = nn.Linear(Dout, V, bias=False)


class TransformerLM(nn.Module):
    """cfg: a TransformerLMConfig (or what it takes); vocab: the dictionary's size; pad / eos / unk: its special ids (fairseq's
    Dictionary: 1, 2, 3).  max_tokens: padded rows (sentences x longest length) per batch of score()."""

    def __init__(self, cfg, vocab, pad=1, eos=2, unk=3, max_tokens=16384):
        super().__init__()
        cfg = cfg if isinstance(cfg, TransformerLMConfig) else TransformerLMConfig(cfg)
        for name in REFUSED:
            if getattr(cfg, name):
                raise NotImplementedError("%s=%r is not built (see unispeech_amd/transformer_lm.py)" % (name, getattr(cfg, name)))
        D, H = cfg.decoder_embed_dim, cfg.decoder_attention_heads
        if D % H or D // H not in (32, 64):
            raise NotImplementedError("decoder_embed_dim=%d / decoder_attention_heads=%d: the attention kernel is built for "
                                      "heads 32 or 64 wide" % (D, H))
        if cfg.activation_fn not in ("relu", "gelu"):
            raise NotImplementedError("activation_fn=%r: relu and gelu are built" % (cfg.activation_fn,))
        self.cfg, self.vocab, self.pad, self.eos, self.unk = cfg, int(vocab), int(pad), int(eos), int(unk)
        self.max_tokens = int(max_tokens)
        self.embed_scale = 1.0 if cfg.no_scale_embedding else math.sqrt(D)
        self.decoder = _Decoder(cfg, self.vocab, self.pad)
        self._image_cache = None
        self.eval()

    # -- loading ---------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True):
        """the reference's state dict with its own keys; quant-noise leaves no keys of its own"""
        self._image_cache = None
        return super().load_state_dict(state_dict, strict=strict)

    def _apply(self, fn, *a, **k):
        self._image_cache = None
        return super()._apply(fn, *a, **k)

    @classmethod
    def from_checkpoint(cls, path, vocab=None, **kw):
        """{"cfg" | "args", "model"} -> the model on the CPU in fp32; the options are a plain dict or a Namespace (a fairseq cfg's
        `model` group is unwrapped).  vocab defaults to the rows of the output projection."""
        ck = torch.load(path, map_location="cpu", weights_only=False)
        if not (isinstance(ck, dict) and "model" in ck and (ck.get("cfg") is not None or ck.get("args") is not None)):
            raise NotImplementedError("%s: only a checkpoint dict {'cfg' | 'args', 'model'} is loaded" % path)
        opts = ck["cfg"] if ck.get("cfg") is not None else ck["args"]
        sd = ck["model"]
        if vocab is None:
            vocab = sd["decoder.output_projection.weight"].shape[0]
        model = cls(TransformerLMConfig(opts), vocab, **kw)
        model.load_state_dict(sd)
        return model

    # -- derived weight images -------------------------------------------------------------------------------------------
    def _images(self):
        """packed q|k|v weights, the scaled input table (adaptive input: every band through its projection, one table) and the
        position table; parameter-sized, built once per (device, dtype)"""
        d = self.decoder
        p0 = d.output_projection.weight
        key = (p0.device, p0.dtype)
        if self._image_cache is not None and self._image_cache[0] == key:
            return self._image_cache[1]
        cfg, im = self.cfg, {}
        with torch.no_grad():
            for i, l in enumerate(d.layers):
                a = l.self_attn
                im["qkv_w%d" % i] = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]).contiguous()
                im["qkv_b%d" % i] = torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]).contiguous()
            if cfg.adaptive_input:
                bands = [(seq[0].weight.float() @ seq[1].weight.float().t()).to(p0.dtype) for seq in d.embed_tokens.embeddings]
                table = torch.cat(bands)
            else:
                table = d.embed_tokens.weight
            im["embed"] = (table.float() * self.embed_scale).to(p0.dtype).contiguous()
        self._image_cache = (key, im)
        return im

    def _positions(self, im, T):
        """the position table that covers T tokens, in the parameters' dtype on their device"""
        cfg, d = self.cfg, self.decoder
        if cfg.no_token_positional_embeddings:
            return None
        if cfg.decoder_learned_pos:
            return d.embed_positions.weight
        need = self.pad + 1 + T
        if im.get("pos_n", 0) < need:
            p0 = d.output_projection.weight
            n = max(need, 2 * im.get("pos_n", 0), self.pad + 1 + 64)
            im["pos"] = sinusoidal_table(n, cfg.decoder_embed_dim, self.pad).to(device=p0.device, dtype=p0.dtype).contiguous()
            im["pos_n"] = n
        return im["pos"]

    # -- the network -----------------------------------------------------------------------------------------------------
    def _check(self, sentences):
        for s in sentences:
            for w in s:
                if not 0 <= int(w) < self.vocab:
                    raise ValueError("word id %r is not one of the %d dictionary entries" % (w, self.vocab))
            if self.cfg.decoder_learned_pos and not self.cfg.no_token_positional_embeddings and \
                    len(s) + 1 > self.cfg.max_target_positions:
                raise ValueError("a sentence of %d words (+ eos) is longer than max_target_positions = %d of the learned "
                                 "positions" % (len(s), self.cfg.max_target_positions))

    def _hidden(self, tokens, lengths):
        """tokens int32 [B, T] on the device, right-padded with pad; lengths int32 [B] -> the decoder's features [B * T,
        decoder_output_dim] (extract_features, transformer.py:846-963); rows beyond a length hold nothing of use"""
        from . import ops
        B, T = tokens.shape
        H = self.cfg.decoder_attention_heads
        ar = torch.arange(T, dtype=torch.int32, device=tokens.device).unsqueeze(0)
        pidx = torch.where(ar < lengths.unsqueeze(1), ar + (self.pad + 1), torch.full_like(ar, self.pad)).reshape(-1)
        return self._stack(tokens.reshape(-1), pidx.contiguous(), T,
                           lambda i, qkv: ops.attn_causal_fwd(qkv.view(B, T, -1), H, lengths).view(B * T, -1))

    def _stack(self, flat, pidx, T, attention):
        """the decoder over M rows that meet only in `attention(layer, qkv [M, 3 D]) -> [M, D]`: flat int32 [M] the tokens, pidx
        int32 [M] their rows of the position table, which covers T tokens"""
        from . import ops
        cfg, d, im = self.cfg, self.decoder, self._images()
        M, D = flat.numel(), cfg.decoder_embed_dim
        dev, dtype = flat.device, d.output_projection.weight.dtype
        new = lambda *shape: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731

        def linear(x, w, b, K, N, epi=0, res=None):
            y = new(M, N)
            ops.gemm(x, w, y, M, N, K, lda=K, ldb=K, ldc=N, bias=b, epi=epi, res=res, ld_res=N if res is not None else 0)
            return y

        def ln(x, r, mod):
            return ops.layernorm_fwd(x, r, mod.weight, mod.bias, mod.eps, save=False)[0]

        x = ops.gather_rows(im["embed"], flat, M)
        if hasattr(d, "project_in_dim"):
            x = linear(x, d.project_in_dim.weight, None, x.shape[1], D)
        pos = self._positions(im, T)
        if pos is not None:
            ops.axpby_(x, ops.gather_rows(pos, pidx, M), 1.0, 1.0)
        if cfg.layernorm_embedding:
            x = ln(x, None, d.layernorm_embedding)
        pre, F = cfg.decoder_normalize_before, cfg.decoder_ffn_embed_dim
        for i, l in enumerate(d.layers):
            a = l.self_attn
            h = ln(x, None, l.self_attn_layer_norm) if pre else x
            qkv = linear(h, im["qkv_w%d" % i], im["qkv_b%d" % i], D, 3 * D)
            o = attention(i, qkv)
            if pre:
                x = linear(o, a.out_proj.weight, a.out_proj.bias, D, D, res=x)
                h = ln(x, None, l.final_layer_norm)
            else:
                x = ln(x, linear(o, a.out_proj.weight, a.out_proj.bias, D, D), l.self_attn_layer_norm)
                h = x
            if cfg.activation_fn == "gelu":
                f = linear(h, l.fc1.weight, l.fc1.bias, D, F, epi=1)
            else:
                f = ops.act_fwd(linear(h, l.fc1.weight, l.fc1.bias, D, F), "relu")
            if pre:
                x = linear(f, l.fc2.weight, l.fc2.bias, F, D, res=x)
            else:
                x = ln(x, linear(f, l.fc2.weight, l.fc2.bias, F, D), l.final_layer_norm)
        if hasattr(d, "layer_norm"):
            x = ln(x, None, d.layer_norm)
        if hasattr(d, "project_out_dim"):
            x = linear(x, d.project_out_dim.weight, None, D, cfg.decoder_output_dim)
        return x

    def batches(self, lengths):
        """indices sorted by length (ties by index), cut where sentences x longest length would pass max_tokens"""
        order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
        out, cur = [], []
        for i in order:
            if cur and lengths[i] * (len(cur) + 1) > self.max_tokens:
                out.append(cur)
                cur = []
            cur.append(i)
        if cur:
            out.append(cur)
        return out

    def score(self, sentences):
        """sentences: lists of word ids -> (token_logprobs fp32 [N, Tmax], totals fp32 [N]) on the CPU; Tmax = longest + 1, the
        entry after a sentence's last word is its eos; entries beyond are 0"""
        from . import ops
        sentences = [[int(w) for w in s] for s in sentences]
        self._check(sentences)
        N = len(sentences)
        Tmax = max([len(s) for s in sentences], default=0) + 1
        out = torch.zeros(N, Tmax, dtype=torch.float32)
        if N == 0:
            return out, out.sum(1)
        w = self.decoder.output_projection.weight
        dev = ops._dev(w)
        with torch.no_grad():
            for batch in self.batches([len(s) + 1 for s in sentences]):
                B, T = len(batch), max(len(sentences[i]) + 1 for i in batch)
                tok = torch.full((B, T), self.pad, dtype=torch.int32)
                tgt = torch.full((B, T), -1, dtype=torch.int32)
                for r, i in enumerate(batch):
                    s = sentences[i]
                    tok[r, :len(s) + 1] = torch.tensor([self.eos] + s, dtype=torch.int32)
                    tgt[r, :len(s) + 1] = torch.tensor(s + [self.eos], dtype=torch.int32)
                lengths = torch.tensor([len(sentences[i]) + 1 for i in batch], dtype=torch.int32)
                x = self._hidden(tok.to(dev), lengths.to(dev))
                rows = torch.nonzero(tgt.reshape(-1) >= 0).reshape(-1).to(torch.int32)
                xs = ops.gather_rows(x, rows.to(dev), rows.numel())      # only the rows that have a target
                lp = lm_logprob(xs, w, tgt.reshape(-1)[rows.long()].contiguous().to(dev))[0].cpu()
                k = 0
                for i in batch:
                    n = len(sentences[i]) + 1
                    out[i, :n] = lp[k:k + n]
                    k += n
        for i, s in enumerate(sentences):                                    # w2l_decoder.py:396-397
            for t, wd in enumerate(s + [self.eos]):
                if wd == self.unk:
                    out[i, t] = -math.inf
        return out, out.sum(1)

    def incremental(self, chunk=1024):
        """a store of decoder states over a tree of word histories (IncrementalStates): the first pass of a beam search asks for
        the next-word distribution of many histories that share prefixes, a few more per frame"""
        return IncrementalStates(self, chunk)


def _check_extension(model, depth, words):
    """the new states' tokens count depth + 1 each"""
    for w in words:
        if not 0 <= int(w) < model.vocab:
            raise ValueError("word id %r is not one of the %d dictionary entries" % (w, model.vocab))
    if len(depth) and max(depth) + 1 > model.cfg.max_target_positions:
        raise ValueError("a history of %d tokens is longer than max_target_positions = %d"
                         % (max(depth) + 1, model.cfg.max_target_positions))


class IncrementalStates:
    """TransformerLM.incremental(): incremental decoding with a KV cache shaped as a tree.  A state is a word history [eos, w_1 ..
    w_n]; its id is its cache slot.  Kept per state: the K and V rows of its last token in every layer, the decoder's final
    hidden row and the log-sum-exp of its logits -- so a row of log-probs is one GEMV away and need not be kept.

      start()                    the state of [eos]
      extend(parents, words)     new state ids, one per (parent, word): one row per new state through every layer in one batch
                                 (wavlm_gemm / wavlm_layernorm_fwd / wavlm_act_fwd as in score(), wavlm_attn_step in place of the
                                 causal attention); the position is the state's depth
      logprob_rows(states, columns=None)   fp32 [n, V] (or [n, len(columns)]) natural-log probabilities on the device
      reset()                    drops everything but the start state
    The caches grow in chunks of `chunk` slots (doubling), never per state."""

    def __init__(self, model, chunk=1024):
        self.model, self.chunk = model, int(chunk)
        w = model.decoder.output_projection.weight
        from . import ops
        self.device, self.dtype = ops._dev(w), w.dtype
        cfg = model.cfg
        if not ops.attn_step_supported(cfg.decoder_embed_dim // cfg.decoder_attention_heads, self.dtype):
            raise NotImplementedError("wavlm_attn_step does not take heads %d wide in %s"
                                      % (cfg.decoder_embed_dim // cfg.decoder_attention_heads, self.dtype))
        if not ops.lm_logprob_supported(w.shape[1], model.vocab, self.dtype):
            raise NotImplementedError("wavlm_lm_logprob does not take decoder_output_dim = %d: no lse per state" % w.shape[1])
        self.cap = 0
        self.kc, self.vc, self.hidden, self.lse = [], [], None, None
        self.parent, self.depth, self.chain = [], [], []
        self.evaluated = 0                                       # states put through the network since construction
        self._wcols = None                                       # (columns, the output projection, its rows at those columns)
        self._grow(self.chunk)
        self._run([-1], [model.eos])

    def __len__(self):
        return len(self.parent)

    def _grow(self, need):
        if need <= self.cap:
            return
        cap = max(need, 2 * self.cap)
        cap = (cap + self.chunk - 1) // self.chunk * self.chunk
        cfg, n = self.model.cfg, len(self.parent)

        def grown(old, width, dtype):
            t = torch.zeros((cap, width) if width else (cap,), dtype=dtype, device=self.device)
            if old is not None and n:
                t[:n] = old[:n]
            return t
        L = cfg.decoder_layers
        self.kc = [grown(self.kc[i] if self.kc else None, cfg.decoder_embed_dim, self.dtype) for i in range(L)]
        self.vc = [grown(self.vc[i] if self.vc else None, cfg.decoder_embed_dim, self.dtype) for i in range(L)]
        self.hidden = grown(self.hidden, self.model.decoder.output_projection.weight.shape[1], self.dtype)
        self.lse = grown(self.lse, 0, torch.float32)
        self.cap = cap

    def start(self):
        return 0

    def reset(self):
        del self.parent[1:], self.depth[1:], self.chain[1:]

    def _run(self, parents, words):
        from . import ops
        m, cfg = self.model, self.model.cfg
        R, n0 = len(words), len(self.parent)
        depth = [self.depth[p] + 1 if p >= 0 else 0 for p in parents]
        _check_extension(m, depth, words)
        self._grow(n0 + R)
        chains = [self.chain[p] + [p] if p >= 0 else [] for p in parents]
        Lmax = max(depth) + 1
        anc = torch.zeros((R, max(1, Lmax - 1)), dtype=torch.int32)
        for r, c in enumerate(chains):
            anc[r, :len(c)] = torch.tensor(c, dtype=torch.int32)
        dev = self.device
        anc = anc.to(dev)
        slot = torch.arange(n0, n0 + R, dtype=torch.int32).to(dev)
        lengths = torch.tensor([x + 1 for x in depth], dtype=torch.int32).to(dev)
        flat = torch.tensor([int(w) for w in words], dtype=torch.int32).to(dev)
        pidx = (lengths + m.pad).contiguous()                    # position row pad + 1 + depth
        H = cfg.decoder_attention_heads
        with torch.no_grad():
            x = m._stack(flat, pidx, Lmax, lambda i, qkv: ops.attn_step(qkv, self.kc[i], self.vc[i], slot, anc, lengths, H, Lmax))
            self.hidden[n0:n0 + R] = x
            none = torch.full((R,), -1, dtype=torch.int32, device=dev)
            # the kernel itself, whatever WAVLM_LM_LOGPROB_COMPOSED says: the composed output layer returns no lse
            self.lse[n0:n0 + R] = ops.lm_logprob(x, m.decoder.output_projection.weight, none, want_lse=True)[1]
        self.parent += list(parents)
        self.depth += depth
        self.chain += chains
        self.evaluated += R
        return list(range(n0, n0 + R))

    def extend(self, parents, words):
        parents = [int(p) for p in parents]
        if len(parents) != len(words):
            raise ValueError("%d parents for %d words" % (len(parents), len(words)))
        for p in parents:
            if not 0 <= p < len(self.parent):
                raise ValueError("state %r is not one of the %d states" % (p, len(self.parent)))
        return self._run(parents, words) if parents else []

    def logprob_rows(self, states, columns=None):
        from . import ops
        states = [int(s) for s in states]
        for s in states:
            if not 0 <= s < len(self.parent):
                raise ValueError("state %r is not one of the %d states" % (s, len(self.parent)))
        w, dev, n = self.model.decoder.output_projection.weight, self.device, len(states)
        idx = torch.tensor(states, dtype=torch.int32).to(dev)
        if columns is not None:
            columns = [int(c) for c in columns]
            if columns and not (0 <= min(columns) and max(columns) < self.model.vocab):
                raise ValueError("a column is not one of the %d dictionary entries" % self.model.vocab)
        V = w.shape[0] if columns is None else len(columns)
        if n == 0 or V == 0:
            return torch.zeros((n, V), dtype=torch.float32, device=dev)
        with torch.no_grad():
            x = ops.gather_rows(self.hidden, idx, n)
            if columns is not None:
                if self._wcols is None or self._wcols[0] != columns or self._wcols[1] is not w:     # a scorer asks for one set
                    cols = torch.tensor(columns, dtype=torch.int32).to(dev)
                    self._wcols = (columns, w, ops.gather_rows(w, cols, V))
                w = self._wcols[2]
            ld = (V + 3) // 4 * 4
            logits = torch.empty((n, ld), dtype=torch.float32, device=dev)
            ops.gemm(x, w, logits, n, V, x.shape[1], lda=x.stride(0), ldb=w.stride(0), ldc=ld)
            return logits[:, :V] - self.lse[idx.long()].unsqueeze(1)


def composed_switch():
    return os.environ.get("WAVLM_LM_LOGPROB_COMPOSED", "") not in ("", "0")


def lm_logprob(x, w, target, want_lse=False):
    """the output layer: x [R, D], w [V, D], target int32 [R] -> (logprob fp32 [R], lse fp32 [R] or None).  wavlm_lm_logprob,
    unless WAVLM_LM_LOGPROB_COMPOSED=1 or the kernel does not take the shape: then wavlm_gemm into fp32 logits + wavlm_ce_rows
    over row chunks whose logits fit COMPOSED_BUDGET_BYTES (no lse on that path)."""
    from . import ops
    R, D = x.shape
    V = w.shape[0]
    if not composed_switch() and ops.lm_logprob_supported(D, V, x.dtype):
        return ops.lm_logprob(x, w, target, want_lse)
    if want_lse:
        raise NotImplementedError("the composed output layer (WAVLM_LM_LOGPROB_COMPOSED, or a shape wavlm_lm_logprob does not "
                                  "take) returns no lse")
    dev = ops._dev(x)
    ld = (V + 3) // 4 * 4
    chunk = max(1, min(R, COMPOSED_BUDGET_BYTES // (4 * ld)))
    logits = torch.empty((chunk, ld), dtype=torch.float32, device=dev)
    out = torch.empty(R, dtype=torch.float32, device=dev)
    valid = (target >= 0) & (target < V)
    safe = torch.where(valid, target, torch.zeros_like(target)).contiguous()
    for r0 in range(0, R, chunk):
        n = min(chunk, R - r0)
        ops.gemm(x, w, logits, n, V, D, lda=x.stride(0), ldb=w.stride(0), ldc=ld, a_off=r0 * x.stride(0))
        loss, _ = ops.ce_rows(logits, safe[r0:r0 + n], V, ld, None, 0, 1.0)
        out[r0:r0 + n] = -loss
    out = torch.where(target < 0, torch.zeros_like(out), torch.where(valid, out, torch.full_like(out, math.nan)))
    return out, None


# --------------------------------------------------------------------------------------------------- float64 reference
def _ln64(x, mod):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + mod.eps) * mod.weight.double() + mod.bias.double()


def _lin64(x, mod):
    y = x @ mod.weight.double().t()
    return y + mod.bias.double() if mod.bias is not None else y


def _decoder64(model, tok, first, attend):
    """the decoder in float64 over the T tokens `tok` (a long tensor) at positions first .. first + T - 1, meeting only in
    attend(layer, q [T, D] scaled, k [T, D], v [T, D]) -> [T, D]: -> log-probs [T, V].  The one specification: _forward64 attends
    causally within the T tokens, incremental_reference over the rows its ancestors left behind."""
    cfg, d = model.cfg, model.decoder
    T, D, H = tok.numel(), cfg.decoder_embed_dim, cfg.decoder_attention_heads
    if cfg.adaptive_input:
        x = torch.zeros(T, D, dtype=torch.float64)
        lo = 0
        for seq, hi in zip(d.embed_tokens.embeddings, d.embed_tokens.cutoff):
            sel = (tok >= lo) & (tok < hi)
            if bool(sel.any()):
                x[sel] = seq[0].weight.double()[tok[sel] - lo] @ seq[1].weight.double().t()
            lo = hi
    else:
        x = d.embed_tokens.weight.double()[tok]
    x = model.embed_scale * x
    if hasattr(d, "project_in_dim"):
        x = _lin64(x, d.project_in_dim)
    if not cfg.no_token_positional_embeddings:
        idx = torch.arange(first, first + T) + model.pad + 1     # make_positions: no padding in a single sentence
        tab = d.embed_positions.weight if cfg.decoder_learned_pos else sinusoidal_table(model.pad + 1 + first + T, D, model.pad)
        x = x + tab.double()[idx]
    if cfg.layernorm_embedding:
        x = _ln64(x, d.layernorm_embedding)
    hd = D // H
    pre = cfg.decoder_normalize_before
    for i, l in enumerate(d.layers):
        a = l.self_attn
        h = _ln64(x, l.self_attn_layer_norm) if pre else x
        o = attend(i, _lin64(h, a.q_proj) * hd ** -0.5, _lin64(h, a.k_proj), _lin64(h, a.v_proj))
        x = x + _lin64(o, a.out_proj)
        if not pre:
            x = _ln64(x, l.self_attn_layer_norm)
        h = _ln64(x, l.final_layer_norm) if pre else x
        f = _lin64(h, l.fc1)
        f = torch.relu(f) if cfg.activation_fn == "relu" else 0.5 * f * (1.0 + torch.erf(f / math.sqrt(2.0)))
        x = x + _lin64(f, l.fc2)
        if not pre:
            x = _ln64(x, l.final_layer_norm)
    if hasattr(d, "layer_norm"):
        x = _ln64(x, d.layer_norm)
    if hasattr(d, "project_out_dim"):
        x = _lin64(x, d.project_out_dim)
    return x


def _attend64(q, k, v, H, future=None):
    """softmax(q k^T) v per head: q [Tq, D], k and v [Tk, D]; future: a bool mask [Tq, Tk] of the pairs that do not attend"""
    Tq, Tk, hd = q.shape[0], k.shape[0], q.shape[1] // H
    q, k, v = (t.view(-1, H, hd).transpose(0, 1) for t in (q, k, v))
    s = q @ k.transpose(1, 2)
    if future is not None:
        s = s.masked_fill(future, -math.inf)
    return (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(Tq, H * hd)


def _forward64(model, words):
    """one sentence, no padding: [eos, w_1 .. w_n] -> log-probs [n + 1, V] in float64"""
    tok = torch.tensor([model.eos] + list(words), dtype=torch.long)
    T, H = tok.numel(), model.cfg.decoder_attention_heads
    future = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    x = _decoder64(model, tok, 0, lambda i, q, k, v: _attend64(q, k, v, H, future))
    return torch.log_softmax(x @ model.decoder.output_projection.weight.double().t(), -1)


def score_reference(model, sentences):
    """TransformerLM.score's rules in float64 on the CPU, sentence by sentence (so nothing depends on the batch): ->
    (token_logprobs float64 [N, Tmax], totals float64 [N])"""
    sentences = [[int(w) for w in s] for s in sentences]
    model._check(sentences)
    Tmax = max([len(s) for s in sentences], default=0) + 1
    out = torch.zeros(len(sentences), Tmax, dtype=torch.float64)
    with torch.no_grad():
        for i, s in enumerate(sentences):
            tgt = torch.tensor(s + [model.eos], dtype=torch.long)
            lp = _forward64(model, s).gather(1, tgt.unsqueeze(1)).squeeze(1)
            lp[tgt == model.unk] = -math.inf
            out[i, :tgt.numel()] = lp
    return out, out.sum(1)


class _ReferenceStates:
    """incremental_reference(model): IncrementalStates' interface in float64 on the CPU, one state at a time, through _decoder64
    -- the new token's row through every layer, its attention over the K and V rows its ancestors left behind"""

    def __init__(self, model):
        self.model = model
        self.parent, self.depth, self.kv, self.hidden = [], [], [], []
        self.evaluated = 0
        self._one(-1, model.eos)

    def __len__(self):
        return len(self.parent)

    def start(self):
        return 0

    def reset(self):
        del self.parent[1:], self.depth[1:], self.kv[1:], self.hidden[1:]

    def _one(self, parent, word):
        H = self.model.cfg.decoder_attention_heads
        depth = self.depth[parent] + 1 if parent >= 0 else 0
        chain, p = [], parent
        while p >= 0:
            chain.append(p)
            p = self.parent[p]
        chain.reverse()
        kv = []

        def attend(i, q, k1, v1):
            kv.append((k1, v1))
            return _attend64(q, torch.cat([self.kv[s][i][0] for s in chain] + [k1]),
                             torch.cat([self.kv[s][i][1] for s in chain] + [v1]), H)
        x = _decoder64(self.model, torch.tensor([int(word)], dtype=torch.long), depth, attend)
        self.parent.append(parent)
        self.depth.append(depth)
        self.kv.append(kv)
        self.hidden.append(x)
        self.evaluated += 1
        return len(self.parent) - 1

    def extend(self, parents, words):
        parents = [int(p) for p in parents]
        if len(parents) != len(words):
            raise ValueError("%d parents for %d words" % (len(parents), len(words)))
        for p in parents:
            if not 0 <= p < len(self.parent):
                raise ValueError("state %r is not one of the %d states" % (p, len(self.parent)))
        _check_extension(self.model, [self.depth[p] + 1 for p in parents], words)
        with torch.no_grad():
            return [self._one(p, w) for p, w in zip(parents, words)]

    def logprob_rows(self, states, columns=None):
        w = self.model.decoder.output_projection.weight.double()
        with torch.no_grad():
            if not len(states):
                return torch.zeros(0, w.shape[0] if columns is None else len(columns), dtype=torch.float64)
            lp = torch.cat([torch.log_softmax(self.hidden[int(s)] @ w.t(), -1) for s in states])    # row by row: no row
            #                                                                                  depends on its company
        return lp if columns is None else lp[:, torch.tensor([int(c) for c in columns], dtype=torch.long)]


def incremental_reference(model):
    """TransformerLM.incremental()'s interface in float64 on the CPU: the specification"""
    with torch.no_grad():
        return _ReferenceStates(model)


# --------------------------------------------------------------------------------------------------------- command line
def parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="python -m unispeech_amd.transformer_lm", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("score", help="log-prob, word count and perplexity per line, and the corpus perplexity")
    s.add_argument("lm", help="checkpoint {'cfg' | 'args', 'model'}")
    s.add_argument("dict", help="fairseq dictionary: `WORD COUNT` per line behind <s> <pad> </s> <unk>")
    s.add_argument("file", nargs="?", default=None, help="one sentence per line (default: standard input)")
    s.add_argument("--bf16", action="store_true")
    s.add_argument("--max-tokens", type=int, default=16384)
    s.add_argument("--cpu-reference", action="store_true", help="score with the float64 reference on the CPU")
    return p.parse_args(argv)


def main(argv=None):
    from .ctc import LetterDictionary
    a = parse_args(argv)
    d = LetterDictionary.load(a.dict)
    model = TransformerLM.from_checkpoint(a.lm, len(d), pad=d.pad(), eos=d.eos(), unk=d.unk(), max_tokens=a.max_tokens)
    with (open(a.file, encoding="utf-8") if a.file else sys.stdin) as f:
        lines = f.read().splitlines()
    sents = [[d.index(w) for w in line.split()] for line in lines]
    if a.cpu_reference:
        _, totals = score_reference(model, sents)
    else:
        model = model.cuda()
        if a.bf16:
            model = model.to(torch.bfloat16)
        _, totals = model.score(sents)
    tot, cnt = 0.0, 0
    for s, t in zip(sents, totals.tolist()):
        n = len(s) + 1                                   # eos counts, as fairseq's eval_lm counts it
        print("%.4f\t%d\t%.4f" % (t, len(s), math.exp(-t / n) if math.isfinite(t) else math.inf))
        if math.isfinite(t):
            tot, cnt = tot + t, cnt + n
    print("corpus: %d sentences, %d scored tokens, perplexity %.4f" % (len(sents), cnt, math.exp(-tot / max(cnt, 1))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
