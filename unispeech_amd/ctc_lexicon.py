"""Lexicon-constrained CTC beam search with a word n-gram LM (csrc/ctc_lexbeam.hip, additive to ABI 30): the decoder of the
reference's examples/speech_recognition/w2l_decoder.py with --lexicon -- W2lKenLMDecoder, which is flashlight's LexiconDecoder with
the CTC criterion, log_add=False and SmearingMode.MAX -- the mode in which the letters + 4-gram word LM figures of wav2vec 2.0 /
HuBERT / WavLM / UniSpeech fine-tuning are produced.

  read_lexicon    the `load_words` file format: `word tok tok ...` per line
  Lexicon         the trie over the spellings as flat tables, smeared with the LM's unigram-after-<s> scores; .to(device)
  load_word_lm    an ARPA file as a ctc_lm.NgramLM over the lexicon's words
  lexicon_beam_search_reference   float64, the specification of the kernel and the host path
  lexicon_beam_decode             wavlm_ctc_lexbeam on the device, the reference on the host
  python -m unispeech_amd.ctc_lexicon decode CKPT DICT a.wav ... --lexicon FILE [--lm FILE.arpa]
  python -m unispeech_amd.ctc_lexicon score CKPT DICT MANIFEST.tsv LABELS.ltr --lexicon FILE [--lm FILE.arpa]
  with --beam --beam-size-token --beam-threshold --lm-weight --word-score --unk-weight --sil-weight --nbest
  rescore_nbest / rescore_reference   second pass: the n-best list re-ranked with a Transformer LM (unispeech_amd.transformer_lm)
  under the objective of the reference's W2lFairseqLMDecoder; --rescore-lm LM.pt --rescore-dict DICT.txt --rescore-weight W
  --rescore-word-score S on the command line, together with --nbest N
  NeuralWordLM / fused_lexicon_decode   the Transformer LM inside the first pass (W2lFairseqLMDecoder itself): the search on the
  host, the LM on the device over a KV-cache tree, a beam's worth of new word histories per frame in one batch;
  --fuse-lm LM.pt --fuse-dict DICT.txt on the command line (exclusive with --lm and --rescore-lm)

Tables (node 0 is the root; a node is a prefix of a spelling):
  child_off  int32 [N + 1]   node v's children are child_*[child_off[v] : child_off[v + 1]]
  child_tok  int32 [E]       the tokens that extend v, ascending within a node
  child_node int32 [E]       the node of v + token
  node_max   fp32  [N]       max(v): the maximum of u(w) over v's labels and of max over its children, u(w) = lm(state of <s>, w)
  label_off  int32 [N + 1]   node v's labels are label_word[label_off[v] : label_off[v + 1]]
  label_word int32 [L]       the words whose spelling ends at v, in word-id order
The word LM is ctc_lm.NgramLM(order, entries, symbols=the lexicon's words): its tok_word maps a word id onto the LM's word, a
word the LM does not list onto <unk>.

Not built: KenLM's binary format, log_add=True, the ASG criterion, a token-level LM together with a lexicon (unit_lm, with an
n-gram or a Transformer LM), the search itself on the device when the LM is a Transformer.  (Time
steps: ctc_align.timesteps aligns a hypothesis's tokens.)  The criterion's wer_lexicon / wer_kenlm_model / wer_args stay refused (ctc.CtcCriterion).
"""
import math
import sys

import numpy as np
import torch

from . import ctc
from .ctc_lm import NgramLM, read_arpa

MAX_LABELS = 6                       # flashlight's kTrieMaxLabel: words that may share one spelling
UNK = "<unk>"


def read_lexicon(path, dictionary):
    """(words, spellings) of a lexicon file: the word strings in order of first appearance, <unk> appended if the file does not
    list it, and [(word id, tuple of token ids)] in file order, an exact duplicate counted once.  ValueError with file:line for a
    token that is not a symbol of the dictionary or is its unk, an empty spelling, a spelling that begins with the silence token,
    and a seventh word for one spelling."""
    sil = ctc.silence_token(dictionary)
    words, wid, spellings, seen, shared = [], {}, [], set(), {}
    with open(path, encoding="utf-8") as f:
        lines = f.read().splitlines()
    for no, line in enumerate(lines, 1):
        parts = line.split()
        if not parts:
            continue

        def bad(what):
            return ValueError("%s:%d: %s" % (path, no, what))
        if len(parts) == 1:
            raise bad("the word %r has an empty spelling" % parts[0])
        toks = []
        for sym in parts[1:]:
            t = int(dictionary.index(sym))
            if t == dictionary.unk():
                raise bad("the token %r is not a symbol of the dictionary (or is its unk)" % sym)
            toks.append(t)
        if toks[0] == sil:
            raise bad("a spelling must not begin with the silence token")
        w = wid.setdefault(parts[0], len(words))
        if w == len(words):
            words.append(parts[0])
        key = (w, tuple(toks))
        if key in seen:
            continue
        n = shared.get(key[1], 0) + 1
        if n > MAX_LABELS:
            raise bad("more than %d words share the spelling %r" % (MAX_LABELS, " ".join(parts[1:])))
        shared[key[1]] = n
        seen.add(key)
        spellings.append(key)
    if UNK not in wid:
        words.append(UNK)
    return words, spellings


def load_word_lm(path, words):
    """the ARPA file as an NgramLM whose symbol map is over the lexicon's words"""
    order, entries = read_arpa(path)
    return NgramLM(order, entries, list(words))


class Lexicon:
    """The trie and its smearing on the host; .to(device) gives the torch tensors the kernel takes."""

    def __init__(self, words, spellings, dictionary, lm=None):
        """words: the word strings, one per word id, <unk> among them; spellings: [(word id, token ids)]; lm: an NgramLM built
        with symbols=words, or None (every u(w) is 0)"""
        self.words, self.lm = list(words), lm
        if UNK not in self.words:
            raise ValueError("the lexicon's words must hold %s" % UNK)
        if lm is not None and len(lm.tok_word) != len(self.words):
            raise ValueError("the language model maps %d symbols, the lexicon has %d words" % (len(lm.tok_word), len(self.words)))
        self.unk_word = self.words.index(UNK)
        self.sil = ctc.silence_token(dictionary)
        C = len(dictionary)
        kids, labels = [{}], [[]]
        for w, toks in sorted(set((int(w), tuple(int(t) for t in toks)) for w, toks in spellings)):
            if not 0 <= w < len(self.words):
                raise ValueError("word id %d is not one of the %d words" % (w, len(self.words)))
            if not toks:
                raise ValueError("the word %r has an empty spelling" % self.words[w])
            if toks[0] == self.sil:
                raise ValueError("the spelling of %r begins with the silence token" % self.words[w])
            v = 0
            for t in toks:
                if not 0 <= t < C or t == dictionary.unk():
                    raise ValueError("the token %d in the spelling of %r is not a symbol of the dictionary" % (t, self.words[w]))
                if t not in kids[v]:
                    kids[v][t] = len(kids)
                    kids.append({})
                    labels.append([])
                v = kids[v][t]
            labels[v].append(w)
            if len(labels[v]) > MAX_LABELS:
                raise ValueError("more than %d words share the spelling of %r" % (MAX_LABELS, self.words[w]))
        self.word_unigram = np.asarray([lm.score_word(lm.start, int(lm.tok_word[w]))[0] if lm is not None else 0.0
                                        for w in range(len(self.words))], dtype=np.float64)
        n = len(kids)
        node_max = np.full(n, -math.inf)
        for v in range(n - 1, -1, -1):                 # a child is created after its parent: descending ids see children first
            m = max([self.word_unigram[w] for w in labels[v]] + [node_max[c] for c in kids[v].values()], default=-math.inf)
            node_max[v] = m
        if n == 1:
            node_max[0] = 0.0
        co, ct, cn, lo, lw = [0], [], [], [0], []
        for v in range(n):
            for t in sorted(kids[v]):
                ct.append(t)
                cn.append(kids[v][t])
            co.append(len(ct))
            lw += sorted(labels[v])
            lo.append(len(lw))
        self.child_off = np.asarray(co, dtype=np.int32)
        self.child_tok = np.asarray(ct, dtype=np.int32)
        self.child_node = np.asarray(cn, dtype=np.int32)
        self.node_max = node_max
        self.label_off = np.asarray(lo, dtype=np.int32)
        self.label_word = np.asarray(lw, dtype=np.int32)
        nlab = np.diff(self.label_off)
        nkid = np.diff(self.child_off)
        self.max_labels = int(nlab.max()) if n else 0
        # the candidates a child can give its parent: a descent if it has children, a word per label (or <unk>, if those are on)
        self.max_node_candidates = {}
        for unk in (False, True):
            per_child = (nkid > 0).astype(np.int64) + np.maximum(nlab, 1 if unk else 0)
            csum = np.concatenate([[0], np.cumsum(per_child[self.child_node])])
            self.max_node_candidates[unk] = int((csum[self.child_off[1:]] - csum[self.child_off[:-1]]).max())
        self._dev = {}

    @classmethod
    def load(cls, path, dictionary, lm_path=None):
        """the lexicon file, and the ARPA file if there is one, as a Lexicon (its .lm is the word LM)"""
        words, spellings = read_lexicon(path, dictionary)
        return cls(words, spellings, dictionary, load_word_lm(lm_path, words) if lm_path is not None else None)

    def __len__(self):
        return len(self.node_max)

    def width(self, ktok, unk=False):
        """an upper bound on the candidates of one hypothesis in one frame with `ktok` considered classes, with or without <unk>
        words: the children among them, each with a descent and its labels, or the fullest node of this trie, plus blank, repeat
        and root silence"""
        unk = bool(unk)
        return min(int(ktok) * (1 + max(self.max_labels, 1 if unk else 0)), self.max_node_candidates[unk]) + 3

    def child(self, v, t):
        lo, hi = int(self.child_off[v]), int(self.child_off[v + 1])
        k = lo + int(np.searchsorted(self.child_tok[lo:hi], t))
        return int(self.child_node[k]) if k < hi and self.child_tok[k] == t else -1

    def labels(self, v):
        return [int(w) for w in self.label_word[self.label_off[v]:self.label_off[v + 1]]]

    def to(self, device):
        """the tables as contiguous torch tensors on `device` (built once per device): a dict of the names above"""
        key = str(device)
        if key not in self._dev:
            def t(a, dtype):
                a = np.ascontiguousarray(a, dtype=dtype)
                if a.size == 0:
                    a = np.zeros(1, dtype=dtype)
                return torch.from_numpy(a).to(device)
            self._dev[key] = {"child_off": t(self.child_off, np.int32), "child_tok": t(self.child_tok, np.int32),
                              "child_node": t(self.child_node, np.int32), "node_max": t(self.node_max, np.float32),
                              "label_off": t(self.label_off, np.int32), "label_word": t(self.label_word, np.int32)}
        return self._dev[key]


def _lex_options(word_score, unk_weight):
    ws, us = float(word_score), float(unk_weight)
    if not math.isfinite(ws):
        raise ValueError("word_score must be finite")
    if not (math.isfinite(us) or us == -math.inf):
        raise ValueError("unk_weight must be finite or -inf")
    return ws, us


def lexicon_beam_search_reference(logits, input_lengths, lexicon, blank=0, sil=-1, beam=50, beam_size_token=100,
                                  beam_threshold=25.0, lm_weight=0.2, word_score=1.0, unk_weight=-math.inf, sil_weight=0.0,
                                  nbest=1, normalized=False, prepare=None, unequal_margins=None):
    """The lexicon-constrained CTC beam search in float64: the specification of wavlm_ctc_lexbeam (csrc/ctc_lexbeam.hip) and the
    host path of lexicon_beam_decode.  logits [T, B, C] (each frame's log-sum-exp is subtracted unless `normalized`); the LM is
    lexicon.lm (None: every LM score 0).

    A hypothesis is (score, lm state, trie node, last token, prev_blank, back-pointer); the start is (0, state of <s>, root,
    none, False).  Frame t < input_length[b]: the considered classes are the min(beam_size_token, C) best by emission (ties to
    the lower class).  A candidate of beam entry r with token n has s = score_r + e[t, n] (+ sil_weight if n is `sil`) and is one of
      1. n == blank, always tried: same state and node, prev_blank = True
      2. n == last_r, not prev_blank_r, last_r not none -- a repeat, always tried: same state and node, prev_blank = False
      3. node_r is the root and n == sil (and 2 does not apply), always tried: silence between words, stays at the root
      4. otherwise n must be considered and node_r must have a child c at n.  Slot 0, if c has children: (state_r, c) with
         s + lm_weight * (max(c) - lexmax(node_r)).  Slot 1 + k for the k-th label w of c: (state after w, root) with
         s + lm_weight * (lm(state_r, w) - lexmax(node_r)) + word_score; the back-pointer records w
      5. c has no label and unk_weight > -inf: slot 1 with the word <unk> and unk_weight in place of word_score
    where lexmax(root) = 0 and lexmax(v) = max(v) (the smearing: over a word the terms telescope to lm(state, w), so only the
    pruning depends on them).  Candidates with equal (state, node, token, prev_blank) merge; the best survives, and best
    everywhere is the total order (score descending, parent rank ascending, token ascending, slot ascending).  Everything below
    best_score - beam_threshold is dropped, the first `beam` in that order are kept, and that order is the next frame's rank.  At
    the end only the survivors at the root finish if there is one, else all; lm_weight * lm(state, </s>) is added, they are
    re-ranked (ties keep their rank) and the first `nbest` are returned.  Input length 0: one empty hypothesis, the end score.

    Differences from flashlight's LexiconDecoder, all deliberate: (1) the search does not start from last_token = sil and no
    final sil is appended, as in the lexicon-free search; (2) a word is completed only by a new token -- flashlight runs its
    label loop outside the CTC new-token test and patches the root with a `continue`; the rule above is the CTC-correct one and
    makes the search with an unbounded beam equal the maximum over all frame paths and their parses; (3) a repeat is allowed at
    every node, flashlight offers only sil at the root.

    Returns (hyps, margin, abs_sum): per sample the list of (words, tokens, score), words as ids; the smallest score difference
    that decided a merge, a threshold cut, the beam boundary or the order of the returned n-best (inf if nothing was decided);
    and the sum of the absolute values of the terms of the 1-best's score.

    Two additive hooks, neither of which changes a result: prepare(states), if given, is handed the LM states of the beam at the
    start of every frame and once more before the end scores (fused_lexicon_decode: a neural LM evaluates them in one batch); unequal_margins, a list, receives per
    sample the smallest difference among the decisions between scores that are NOT exactly equal (equal scores -- -inf against
    -inf, one LM entry reached twice -- are settled by the order above whatever the arithmetic)."""
    x = logits.detach().to(torch.float64).cpu().numpy() if torch.is_tensor(logits) else np.asarray(logits, dtype=np.float64)
    T, B, C = x.shape
    beam, ktok, thr, lmw, silw, nbest = ctc._beam_options(C, beam, beam_size_token, beam_threshold, lm_weight, sil_weight, nbest)
    wsc, usc = _lex_options(word_score, unk_weight)
    il = [T] * B if input_lengths is None else [min(max(int(v), 0), T) for v in ctc._host_ints(input_lengths, "input_lengths")]
    if not 0 <= int(blank) < C:
        raise ValueError("blank = %d is not a class" % blank)
    if len(lexicon.child_tok) and int(lexicon.child_tok.max()) >= C:
        raise ValueError("the lexicon spells with token %d, the logits have %d classes" % (int(lexicon.child_tok.max()), C))
    blank, sil = int(blank), int(sil)
    lx, lm = lexicon, lexicon.lm
    nmax = lx.node_max
    has_kids = np.diff(lx.child_off) > 0

    def lm_word(st, w):
        return lm.score_word(st, int(lm.tok_word[w])) if lm is not None else (0.0, st)
    out, margins, sums = [], [], []
    for b in range(B):
        e = x[:il[b], b]
        if not normalized and il[b]:
            m = e.max(-1, keepdims=True)
            e = e - (m + np.log(np.exp(e - m).sum(-1, keepdims=True)))
        if not np.isfinite(e).all():
            raise ValueError("sample %d: the emissions must be finite" % b)
        margin = margin_ne = math.inf

        def decided(diff):
            nonlocal margin, margin_ne
            margin = min(margin, diff)
            if diff > 0:
                margin_ne = min(margin_ne, diff)
        # (score, state, node, token, prev_blank, back = (parent's back, token, word or -1) chain, abs_sum)
        hyps = [(0.0, lm.start if lm is not None else 0, 0, -1, False, None, 0.0)]
        for t in range(il[b]):
            et = e[t]
            if prepare is not None:
                prepare([h[1] for h in hyps])
            considered = set(int(c) for c in np.lexsort((np.arange(C), -et))[:ktok])
            cands = {}

            def put(r, n, slot, s, a, st, nd, word, back):
                key, rank = (st, nd, n), (-s, r, n, slot)           # prev_blank is (n == blank)
                old = cands.get(key)
                if old is not None:
                    decided(abs(old[0][0] - rank[0]))
                if old is None or rank < old[0]:
                    cands[key] = (rank, (s, st, nd, n, n == blank, (back, n, word), a))
            for r, (sc, st, nd, tok, pb, back, ab) in enumerate(hyps):
                lexmax = 0.0 if nd == 0 else float(nmax[nd])
                tried = set(considered)
                tried.add(blank)
                if tok >= 0 and not pb:
                    tried.add(tok)
                if nd == 0 and 0 <= sil < C:
                    tried.add(sil)
                for n in sorted(tried):
                    v = float(et[n])
                    s, a = sc + v, ab + abs(v)
                    if n == sil:
                        s, a = s + silw, a + abs(silw)
                    if n == blank or (n == tok and not pb) or (nd == 0 and n == sil):       # kinds 1, 2, 3
                        put(r, n, 0, s, a, st, nd, -1, back)
                        continue
                    c = lx.child(nd, n) if n in considered else -1
                    if c < 0:
                        continue
                    if has_kids[c]:
                        d = lmw * (float(nmax[c]) - lexmax)
                        put(r, n, 0, s + d, a + abs(d), st, c, -1, back)
                    labs = lx.labels(c)
                    if labs:
                        for k, w in enumerate(labs):
                            l, st2 = lm_word(st, w)
                            d = lmw * (l - lexmax)
                            put(r, n, 1 + k, s + d + wsc, a + abs(d) + abs(wsc), st2, 0, w, back)
                    elif usc > -math.inf:
                        l, st2 = lm_word(st, lx.unk_word)
                        d = lmw * (l - lexmax)
                        put(r, n, 1, s + d + usc, a + abs(d) + abs(usc), st2, 0, lx.unk_word, back)
            best = -min(v[0][0] for v in cands.values())
            if thr != math.inf:
                for v in cands.values():
                    decided(abs(-v[0][0] - (best - thr)))
            keep = sorted((v for v in cands.values() if -v[0][0] >= best - thr), key=lambda v: v[0])
            if len(keep) > beam:
                decided(keep[beam - 1][1][0] - keep[beam][1][0])
            hyps = [v[1] for v in keep[:beam]]
        if prepare is not None:
            prepare([h[1] for h in hyps])                # the end scores
        if any(h[2] == 0 for h in hyps):
            hyps_fin = [(r, h) for r, h in enumerate(hyps) if h[2] == 0]
        else:
            hyps_fin = list(enumerate(hyps))
        fin = []
        for r, h in hyps_fin:
            l = lmw * lm.score_eos(h[1]) if lm is not None else 0.0
            fin.append((-(h[0] + l), r, h, h[6] + abs(l)))
        fin.sort(key=lambda v: v[:2])
        for i in range(min(nbest, len(fin) - 1)):
            decided(fin[i + 1][0] - fin[i][0])
        res = []
        for msc, _, h, _ in fin[:nbest]:
            path, wds, back = [], [], h[5]
            while back is not None:
                path.append(back[1])
                if back[2] >= 0:
                    wds.append(int(back[2]))
                back = back[0]
            seq, last = [], -1
            for a in reversed(path):
                if a != last and a != blank:
                    seq.append(int(a))
                last = a
            res.append((wds[::-1], seq, -msc))
        out.append(res)
        margins.append(margin)
        if unequal_margins is not None:
            unequal_margins.append(margin_ne)
        sums.append(fin[0][3])
    return out, margins, sums


def lexicon_beam_decode(logits, input_lengths, dictionary, lexicon, lm=None, beam=50, beam_size_token=100, beam_threshold=25.0,
                        lm_weight=0.2, word_score=1.0, unk_weight=-math.inf, sil_weight=0.0, nbest=1, normalized=False,
                        blank=None):
    """Lexicon-constrained CTC beam search with an optional word n-gram LM, by the rules of lexicon_beam_search_reference.
    logits [T, B, C], either storage order; lexicon: a Lexicon over this dictionary; lm: the NgramLM the lexicon was built with
    (lexicon.lm), or None for a lexicon without one.  Returns, per sample, a list of at most nbest (word strings, tokens, score),
    best first.

    Device logits take wavlm_ctc_lexbeam (one workgroup per utterance; sizes beyond wavlm_ctc_lexbeam_supported raise
    NotImplementedError naming the argument, before any launch); host logits take the float64 reference."""
    T, B, C = logits.shape
    if blank is None:
        blank = dictionary.bos()
    if lm is not lexicon.lm:
        raise ValueError("lm must be the language model the lexicon was built with (lexicon.lm): the trie is smeared with it")
    sil = ctc.silence_token(dictionary)
    if not (torch.is_tensor(logits) and logits.is_cuda):
        hyps = lexicon_beam_search_reference(logits, input_lengths, lexicon, blank, sil, beam, beam_size_token, beam_threshold,
                                             lm_weight, word_score, unk_weight, sil_weight, nbest, normalized)[0]
        return [[([lexicon.words[w] for w in wds], toks, sc) for wds, toks, sc in h] for h in hyps]
    from . import ops
    beam, ktok, thr, lmw, silw, nbest = ctc._beam_options(C, beam, beam_size_token, beam_threshold, lm_weight, sil_weight, nbest)
    wsc, usc = _lex_options(word_score, unk_weight)
    nbest = min(nbest, beam)
    dev = logits.device
    x = logits.detach().transpose(0, 1)
    if x.shape[2] > 1 and x.stride(2) != 1:
        x = x.contiguous()
    if input_lengths is None:
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
    else:
        il = torch.as_tensor(input_lengths).to(device=dev, dtype=torch.int32).contiguous()
    res = ops.ctc_lexbeam(x, il, blank, sil, lexicon, beam, ktok, thr, lmw, wsc, usc, silw, nbest, normalized)
    tokens, counts, scores, n_hyp, words, wcounts = (v.cpu().numpy() for v in res)
    return [[([lexicon.words[int(w)] for w in words[b, h, :wcounts[b, h]]], [int(v) for v in tokens[b, h, :counts[b, h]]],
              float(scores[b, h])) for h in range(int(n_hyp[b]))] for b in range(B)]


# ------------------------------------------------------------------------------- a Transformer LM inside the first pass
class NeuralWordLM:
    """A transformer_lm.TransformerLM as the word LM of the lexicon search: the protocol ctc_lm.NgramLM gives the lexicon code
    (start, tok_word, words, score_word(state, id) -> (score, state), score_eos(state)) with the conventions of the reference's
    FairseqLM (examples/speech_recognition/w2l_decoder.py:288-415): natural log, a lexicon word the LM's dictionary lacks is
    its unk, and unk scores -inf.  A state is a word history; a history reached twice is one state.

    lm_or_reference: a TransformerLM on the device (its .incremental() is used) or a state store with that interface
    (transformer_lm.incremental_reference(model): float64 on the CPU).  lm_dictionary: the LM's dictionary.  words: the lexicon's
    word strings, one per word id.

    score_word names the state after the word without running the network; a state is evaluated when a score is first asked of
    it.  prepare(states) evaluates, in one batched extend() per depth, every listed state that has no row yet -- the search hands
    it the beam at the start of a frame.  Of a row of log-probs only the lexicon's columns (the LM entries of its words, and eos)
    are computed and brought to the host, in float64; prepare(states, only=True) forgets the rows of states that left the beam
    and drop_rows() all of them (each is rebuilt by one GEMV from the state's hidden row); empty_cache() forgets every state but the start, per utterance as the
    reference does."""

    def __init__(self, lm_or_reference, lm_dictionary, words):
        self.store = lm_or_reference if hasattr(lm_or_reference, "extend") else lm_or_reference.incremental()
        self.words = list(words)
        self.unk, self.eos = int(lm_dictionary.unk()), int(lm_dictionary.eos())
        self.tok_word = np.asarray([int(lm_dictionary.index(w)) for w in self.words], dtype=np.int64)
        self.columns = sorted(set(int(t) for t in self.tok_word) | {self.eos})     # the only entries of a row the search can ask for
        self._col = {t: i for i, t in enumerate(self.columns)}
        self.start = 0
        self.calls = 0                                   # extend() calls since construction
        self._parent, self._word, self._slot, self._kids, self._rows = [-1], [self.eos], [self.store.start()], [{}], {}

    @property
    def evaluated(self):
        """states put through the network since construction (the start included)"""
        return self.store.evaluated

    def empty_cache(self):
        self.store.reset()
        start_row = self._rows.get(0)
        del self._parent[1:], self._word[1:], self._slot[1:], self._kids[1:]
        self._kids[0] = {}
        self._rows = {} if start_row is None else {0: start_row}

    def drop_rows(self):
        self._rows = {}

    def prepare(self, states, only=False):
        """only: forget the rows of every other state but the start (the search passes its whole beam: a state that left it is
        never asked again, and a row costs len(columns) float64 on the host)"""
        if only:
            keep = set(int(s) for s in states) | {self.start}
            self._rows = {s: r for s, r in self._rows.items() if s in keep}
        todo, seen = [], set()
        for s in states:
            s = int(s)
            while s not in seen and self._slot[s] is None:          # an unevaluated parent comes first
                seen.add(s)
                todo.append(s)
                s = self._parent[s]
        by_depth = {}
        for s in todo:
            d, p = 0, s
            while self._slot[p] is None:
                d, p = d + 1, self._parent[p]
            by_depth.setdefault(d, []).append(s)
        for d in sorted(by_depth):
            level = sorted(by_depth[d])
            new = self.store.extend([self._slot[self._parent[s]] for s in level], [self._word[s] for s in level])
            self.calls += 1
            for s, slot in zip(level, new):
                self._slot[s] = slot
        need = sorted(set(int(s) for s in states) - set(self._rows))
        if need:
            rows = self.store.logprob_rows([self._slot[s] for s in need], self.columns).detach().cpu().to(torch.float64).numpy()
            for s, row in zip(need, rows):
                self._rows[s] = row

    def _row(self, state):
        if state not in self._rows:
            self.prepare([state])
        return self._rows[state]

    def score_word(self, state, word):
        state, word = int(state), int(word)
        child = self._kids[state].get(word)
        if child is None:
            child = self._kids[state][word] = len(self._parent)
            self._parent.append(state)
            self._word.append(word)
            self._slot.append(None)
            self._kids.append({})
        if word not in self._col:
            raise ValueError("word id %d is not an entry of tok_word" % word)
        return (-math.inf if word == self.unk else float(self._row(state)[self._col[word]])), child

    def score_eos(self, state):
        return float(self._row(int(state))[self._col[self.eos]])


def fused_lexicon_decode(logits, input_lengths, dictionary, lexicon, lm, beam=50, beam_size_token=100, beam_threshold=25.0,
                         lm_weight=0.2, word_score=1.0, unk_weight=-math.inf, sil_weight=0.0, nbest=1, normalized=False,
                         blank=None, stats=None):
    """The lexicon search with a Transformer LM inside the first pass -- the reference's W2lFairseqLMDecoder
    (examples/speech_recognition/w2l_decoder.py:417-531): the LM scores every word as the search completes it and the trie is
    smeared with its row at the start state.  lm: the NeuralWordLM the lexicon was built with (lexicon.lm).  The rules are
    lexicon_beam_search_reference's to the letter -- that function runs, on the host in float64, as flashlight's search runs on
    the host -- with one addition: each frame first hands the beam's LM states to lm.prepare, so the network evaluates a beam's
    worth of new word histories per frame in one batch over its KV-cache tree instead of one prefix at a time.  The emissions
    come to the host once; the LM's cache is emptied per utterance.  stats, a dict, receives per utterance the states evaluated
    and the extend() calls.  Returns, per sample, a list of at most nbest (word strings, tokens, score), best first."""
    T, B, C = logits.shape
    if blank is None:
        blank = dictionary.bos()
    if lm is not lexicon.lm or not hasattr(lm, "prepare"):
        raise ValueError("lm must be the NeuralWordLM the lexicon was built with (lexicon.lm): the trie is smeared with it")
    sil = ctc.silence_token(dictionary)
    x = logits.detach().to(torch.float64).cpu().numpy() if torch.is_tensor(logits) else np.asarray(logits, dtype=np.float64)
    il = [T] * B if input_lengths is None else ctc._host_ints(input_lengths, "input_lengths")
    out = []
    for b in range(B):
        lm.empty_cache()
        n0, c0 = lm.evaluated, lm.calls
        hyps = lexicon_beam_search_reference(x[:, b:b + 1], [il[b]], lexicon, blank, sil, beam, beam_size_token, beam_threshold,
                                             lm_weight, word_score, unk_weight, sil_weight, nbest, normalized,
                                             prepare=lambda states: lm.prepare(states, only=True))[0][0]
        out.append([([lexicon.words[w] for w in wds], toks, sc) for wds, toks, sc in hyps])
        if stats is not None:
            stats.setdefault("states", []).append(lm.evaluated - n0)
            stats.setdefault("calls", []).append(lm.calls - c0)
    return out


# ------------------------------------------------------------------------------------------------------------ rescoring
def ngram_sum(lm, words):
    """S_ngram: what the first pass added for this word sequence before the LM weight -- sum of log10 p(w_i | history) from the
    state of <s>, plus the sentence end -- in the search's own units.  words: strings, or the lexicon's word ids (the symbols the
    NgramLM was built over); a word the LM does not list scores as its <unk>.  0 without a first-pass LM."""
    if lm is None:
        return 0.0
    ids = lm.__dict__.get("_word_ids")
    if ids is None:
        ids = lm._word_ids = {w: i for i, w in enumerate(lm.words)}
    st, total = lm.start, 0.0
    for w in words:
        wid = ids.get(w, ids[UNK]) if isinstance(w, str) else int(lm.tok_word[int(w)])
        l, st = lm.score_word(st, wid)
        total += l
    return total + lm.score_eos(st)


def _rescore(hyps, scorer, lm_dictionary, first_pass_lm, lm_weight, word_score, rescore_weight, rescore_word_score):
    seqs, index = [], {}
    for utt in hyps:
        for h in utt:
            key = tuple(int(lm_dictionary.index(w)) for w in h[0])      # by spelling; unknown to the LM -> its unk
            if key not in index:
                index[key] = len(seqs)
                seqs.append(list(key))
    totals = [float(v) for v in scorer(seqs)[1]] if seqs else []       # each distinct word sequence once
    rw, out = float(rescore_weight), []
    for utt in hyps:
        res = []
        for h in utt:
            words, tokens, s1 = h[0], h[1], float(h[2])
            tl = totals[index[tuple(int(lm_dictionary.index(w)) for w in words)]]
            s2 = s1 - float(lm_weight) * ngram_sum(first_pass_lm, words) + (rw * tl if rw != 0.0 else 0.0) \
                + (float(rescore_word_score) - float(word_score)) * len(words)
            res.append({"words": list(words), "tokens": list(tokens), "score": s2, "lm_score": tl, "first_pass_score": s1})
        out.append(sorted(res, key=lambda e: -e["score"]))              # stable: ties and all -inf keep first-pass order
    return out


def rescore_nbest(hyps, lm, lm_dictionary, first_pass_lm=None, lm_weight=0.0, word_score=0.0, rescore_weight=1.0,
                  rescore_word_score=0.0):
    """Second pass over the n-best lists of lexicon_beam_decode(..., nbest=N) with a transformer_lm.TransformerLM on the device:
    every hypothesis's first-pass score s1 becomes
        s2 = s1 - lm_weight * S_ngram(words) + rescore_weight * S_tlm(words) + (rescore_word_score - word_score) * len(words)
    -- the objective of the reference's W2lFairseqLMDecoder (AM + lm_weight x LM + word_score x words + silence terms) evaluated on
    that hypothesis, restricted to the list.  lm_weight / word_score: the first pass's options, first_pass_lm its NgramLM (None: it
    had none); S_tlm: TransformerLM.score's total in natural log, as the reference feeds it to flashlight; words are mapped onto
    lm_dictionary by spelling, one the LM does not know is its unk and scores -inf.  Returns, per utterance, the list re-sorted by
    s2 (stable) as dicts with words, tokens, score, lm_score and first_pass_score."""
    return _rescore(hyps, lm.score, lm_dictionary, first_pass_lm, lm_weight, word_score, rescore_weight, rescore_word_score)


def rescore_reference(hyps, lm, lm_dictionary, first_pass_lm=None, lm_weight=0.0, word_score=0.0, rescore_weight=1.0,
                      rescore_word_score=0.0):
    """rescore_nbest in float64 over transformer_lm.score_reference: the specification"""
    from .transformer_lm import score_reference
    return _rescore(hyps, lambda s: score_reference(lm, s), lm_dictionary, first_pass_lm, lm_weight, word_score, rescore_weight,
                    rescore_word_score)


# ---------------------------------------------------------------------------------------------------------- command line
def parse_args(argv=None):
    p, d, c = ctc.base_parser("python -m unispeech_amd.ctc_lexicon", __doc__.split("\n\n")[0],
                              "word transcripts of the lexicon beam search, one line per file",
                              "UER / WER of the lexicon beam search over a manifest")
    for q in (d, c):
        q.add_argument("--lexicon", required=True, metavar="FILE", help="`word tok tok ...` per line")
        ctc.add_beam_options(q, "n-gram word LM (ARPA text) over the lexicon's words")
        q.add_argument("--word-score", type=float, default=1.0)
        q.add_argument("--unk-weight", type=float, default=-math.inf)
        q.add_argument("--rescore-lm", default=None, metavar="LM.pt", help="Transformer LM checkpoint: re-rank the --nbest list")
        q.add_argument("--rescore-dict", default=None, metavar="DICT.txt", help="the Transformer LM's fairseq dictionary")
        q.add_argument("--rescore-weight", type=float, default=1.0)
        q.add_argument("--rescore-word-score", type=float, default=None, help="default: --word-score")
        q.add_argument("--fuse-lm", default=None, metavar="LM.pt",
                       help="Transformer LM checkpoint: the word LM of the first pass (natural log; --lm-weight applies)")
        q.add_argument("--fuse-dict", default=None, metavar="DICT.txt", help="the fused Transformer LM's fairseq dictionary")
    a = ctc.refuse_binary_lm(p.parse_args(argv))
    if (a.rescore_lm is None) != (a.rescore_dict is None):
        p.error("--rescore-lm and --rescore-dict go together")
    if (a.fuse_lm is None) != (a.fuse_dict is None):
        p.error("--fuse-lm and --fuse-dict go together")
    if a.fuse_lm is not None and a.lm is not None:
        p.error("--fuse-lm and --lm are exclusive: the first pass has one word LM")
    if a.fuse_lm is not None and a.rescore_lm is not None:
        p.error("--fuse-lm and --rescore-lm are exclusive: a fused Transformer LM leaves no second pass")
    return a


def _options(a):
    return dict(ctc._beam_kwargs(a), word_score=a.word_score, unk_weight=a.unk_weight)


def main(argv=None):
    a = parse_args(argv)
    d = ctc.LetterDictionary.load(a.dict)
    kw = _options(a)
    tlm = None
    if a.fuse_lm is not None:
        from .transformer_lm import TransformerLM
        fd = ctc.LetterDictionary.load(a.fuse_dict)
        flm = TransformerLM.from_checkpoint(a.fuse_lm, len(fd), pad=fd.pad(), eos=fd.eos(), unk=fd.unk()).cuda()
        if a.bf16:
            flm = flm.to(torch.bfloat16)
        words, spellings = read_lexicon(a.lexicon, d)
        lexicon = Lexicon(words, spellings, d, NeuralWordLM(flm, fd, words))
    else:
        lexicon = Lexicon.load(a.lexicon, d, a.lm)
    if a.rescore_lm is not None:
        from .transformer_lm import TransformerLM
        ld = ctc.LetterDictionary.load(a.rescore_dict)
        tlm = TransformerLM.from_checkpoint(a.rescore_lm, len(ld), pad=ld.pad(), eos=ld.eos(), unk=ld.unk()).cuda()
        if a.bf16:
            tlm = tlm.to(torch.bfloat16)
        rws = a.word_score if a.rescore_word_score is None else a.rescore_word_score

    def search(logits, il, d):                  # the first pass, and the second if a Transformer LM was given
        if a.fuse_lm is not None:
            return fused_lexicon_decode(logits, il, d, lexicon, lexicon.lm, **kw)
        hyps = lexicon_beam_decode(logits, il, d, lexicon, lexicon.lm, **kw)
        if tlm is None:
            return hyps
        res = rescore_nbest(hyps, tlm, ld, lexicon.lm, a.lm_weight if lexicon.lm is not None else 0.0, a.word_score,
                            a.rescore_weight, rws)
        return [[(e["words"], e["tokens"], e["score"]) for e in utt] for utt in res]
    if a.cmd == "score":
        def decoder(logits, il, d):
            return [(h[0][1], h[0][0]) if h else ([], []) for h in search(logits, il, d)]
        return ctc.score(a, decoder)

    def lines(logits, d):                       # one line per hypothesis, best first; with --nbest above 1 the score in front
        for words, _, sc in search(logits, None, d)[0]:
            text = " ".join(words)
            yield text if a.nbest == 1 else "%.4f\t%s" % (sc, text)
    return ctc.decode(a, lines)


if __name__ == "__main__":
    sys.exit(main())
