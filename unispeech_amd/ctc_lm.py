"""n-gram unit language model for the CTC beam search (ctc.beam_decode, csrc/ctc_beam.hip): an ARPA text reader and the flat
tables the kernel walks.  No KenLM, no binary format: `NgramLM.load(path, dictionary)` reads the text file.

Scores are the file's own (log10), as KenLM's BaseScore returns them.  Backoff is Katz's: from the state h look up h + w; on a
miss add backoff(h), drop the oldest word and repeat; a context that is not an entry contributes backoff 0.  The state after
scoring is the longest suffix, of at most order - 1 words, of the matched n-gram that is itself an entry.

Tables.  A node is a word sequence: every entry of the file, and every prefix and suffix of one (a file need be neither prefix-
nor suffix-closed; a node that is not an entry has backoff 0 and is never a state).  Node 0 is the empty sequence.
  child_off   int32 [N + 1]  node h's children are child_*[child_off[h] : child_off[h + 1]]
  child_word  int32 [E]      the words w for which h + w is an entry, ascending within a node
  child_logp  fp32  [E]      log10 p(w | h)
  child_next  int32 [E]      the state after h + w
  node_backoff fp32 [N]      backoff(h), 0 where the file gives none
  node_suffix int32 [N]      the node of h without its oldest word (0 for node 0)
  tok_word    int32 [C]      dictionary id -> word, by the symbol's string; a symbol the file does not list is <unk>
`start` is the state of <s>, `eos_word` the word </s>.  The host keeps float64 copies (score() is the reference's LM).
"""
import bisect
import re

import numpy as np

MAX_ORDER = 6


def _symbol(dictionary, i):
    syms = getattr(dictionary, "symbols", None)
    return syms[i] if syms is not None else dictionary[i]


def read_arpa(path):
    """(order, {tuple of words: (log10 p, backoff)}) of an ARPA file; ValueError naming the line of anything malformed"""
    with open(path, encoding="utf-8") as f:
        lines = f.read().splitlines()

    def bad(no, what):
        return ValueError("%s:%d: %s" % (path, no, what))
    no = 0
    while no < len(lines) and lines[no].strip() != "\\data\\":
        if lines[no].strip():
            raise bad(no + 1, "expected \\data\\")
        no += 1
    if no == len(lines):
        raise bad(len(lines) or 1, "no \\data\\ section")
    no += 1
    counts = {}
    while no < len(lines) and not lines[no].startswith("\\"):
        s = lines[no].strip()
        if s:
            m = re.fullmatch(r"ngram\s+(\d+)\s*=\s*(\d+)", s)
            if not m:
                raise bad(no + 1, "expected `ngram N=COUNT`")
            counts[int(m.group(1))] = int(m.group(2))
        no += 1
    order = len(counts)
    if order < 1 or sorted(counts) != list(range(1, order + 1)):
        raise bad(no, "the ngram counts must list the orders 1 .. N")
    if order > MAX_ORDER:
        raise bad(no, "order %d: orders 1 to %d are read" % (order, MAX_ORDER))
    entries = {}
    for k in range(1, order + 1):
        while no < len(lines) and not lines[no].strip():
            no += 1
        if no == len(lines) or lines[no].strip() != "\\%d-grams:" % k:
            raise bad(min(no, len(lines) - 1) + 1, "expected \\%d-grams:" % k)
        no += 1
        seen = 0
        while no < len(lines) and not lines[no].startswith("\\"):
            s = lines[no].strip()
            if s:
                parts = s.split()
                if len(parts) not in (k + 1, k + 2):
                    raise bad(no + 1, "a %d-gram line holds a score, %d words and at most one backoff" % (k, k))
                try:
                    logp = float(parts[0])
                    bo = float(parts[k + 1]) if len(parts) == k + 2 else 0.0
                except ValueError:
                    raise bad(no + 1, "not a number") from None
                if not (np.isfinite(logp) and np.isfinite(bo)):
                    raise bad(no + 1, "scores and backoffs must be finite")
                g = tuple(parts[1:k + 1])
                if g in entries:
                    raise bad(no + 1, "the n-gram is listed twice")
                entries[g] = (logp, bo)
                seen += 1
            no += 1
        if seen != counts[k]:
            raise bad(no, "\\%d-grams: holds %d entries, the header says %d" % (k, seen, counts[k]))
    while no < len(lines) and not lines[no].strip():
        no += 1
    if no == len(lines) or lines[no].strip() != "\\end\\":
        raise bad(min(no, len(lines) - 1) + 1, "expected \\end\\")
    for w in ("<unk>", "<s>", "</s>"):
        if (w,) not in entries:
            raise bad(no + 1, "the unigrams do not list %s" % w)
    for g in entries:
        for w in g:
            if (w,) not in entries:
                raise bad(no + 1, "the word %r of an n-gram is not a unigram" % w)
    return order, entries


class NgramLM:
    """The tables above on the host; .to(device) gives the torch tensors the kernel takes."""

    def __init__(self, order, entries, symbols):
        """entries: {tuple of words: (log10 p, backoff)} holding the unigrams <unk>, <s>, </s>; symbols: the dictionary's strings,
        one per class id"""
        self.order, self.entries = int(order), dict(entries)
        words = sorted(g[0] for g in entries if len(g) == 1)
        wid = {w: i for i, w in enumerate(words)}
        self.words = words
        nodes = {()}
        for g in entries:
            for a in range(len(g) + 1):
                for b in range(a, len(g) + 1):
                    nodes.add(g[a:b])                  # every contiguous piece: prefixes of suffixes
        order_of = sorted(nodes, key=lambda g: (len(g), [wid[w] for w in g]))
        nid = {g: i for i, g in enumerate(order_of)}

        def state_of(g):
            g = g[-(self.order - 1):] if self.order > 1 else ()
            while g and g not in entries:
                g = g[1:]
            return nid[g]
        kids = [[] for _ in order_of]
        for g, (logp, _) in entries.items():
            kids[nid[g[:-1]]].append((wid[g[-1]], logp, state_of(g)))
        off, cw, cl, cn = [0], [], [], []
        for k in kids:
            k.sort()
            cw += [w for w, _, _ in k]
            cl += [p for _, p, _ in k]
            cn += [s for _, _, s in k]
            off.append(len(cw))
        self.child_off = np.asarray(off, dtype=np.int32)
        self.child_word = np.asarray(cw, dtype=np.int32)
        self.child_logp = np.asarray(cl, dtype=np.float64)
        self.child_next = np.asarray(cn, dtype=np.int32)
        self.node_backoff = np.asarray([entries[g][1] if g in entries else 0.0 for g in order_of], dtype=np.float64)
        self.node_suffix = np.asarray([nid[g[1:]] for g in order_of], dtype=np.int32)
        self.tok_word = np.asarray([wid.get(s, wid["<unk>"]) for s in symbols], dtype=np.int32)
        self.start = state_of(("<s>",))
        self.eos_word = wid["</s>"]
        self._nid = nid
        self._dev = {}

    @classmethod
    def load(cls, path, dictionary):
        order, entries = read_arpa(path)
        return cls(order, entries, [_symbol(dictionary, i) for i in range(len(dictionary))])

    def __len__(self):
        return len(self.node_suffix)

    def state_of(self, words):
        """the state after the words (strings): the longest suffix of at most order - 1 of them that is an entry"""
        g = tuple(words)[-(self.order - 1):] if self.order > 1 else ()
        while g and g not in self.entries:
            g = g[1:]
        return self._nid[g]

    def score_word(self, state, word):
        """(log10 p(word | state), next state) for a word id"""
        acc, node = 0.0, int(state)
        while True:
            lo, hi = int(self.child_off[node]), int(self.child_off[node + 1])
            k = bisect.bisect_left(self.child_word, word, lo, hi)
            if k < hi and self.child_word[k] == word:
                return acc + float(self.child_logp[k]), int(self.child_next[k])
            if node == 0:
                raise KeyError("word %d has no unigram" % word)
            acc += float(self.node_backoff[node])
            node = int(self.node_suffix[node])

    def score(self, state, token):
        """(log10 p(token | state), next state) for a dictionary id"""
        return self.score_word(state, int(self.tok_word[token]))

    def score_eos(self, state):
        return self.score_word(state, self.eos_word)[0]

    def to(self, device):
        """the tables as contiguous torch tensors on `device` (built once per device): a dict of the names above"""
        import torch
        key = str(device)
        if key not in self._dev:
            def t(a, dtype):
                a = np.ascontiguousarray(a, dtype=dtype)
                if a.size == 0:
                    a = np.zeros(1, dtype=dtype)
                return torch.from_numpy(a).to(device)
            self._dev[key] = {"child_off": t(self.child_off, np.int32), "child_word": t(self.child_word, np.int32),
                              "child_logp": t(self.child_logp, np.float32), "child_next": t(self.child_next, np.int32),
                              "node_backoff": t(self.node_backoff, np.float32), "node_suffix": t(self.node_suffix, np.int32),
                              "tok_word": t(self.tok_word, np.int32)}
        return self._dev[key]


def write_arpa(path, order, entries):
    """the entries as an ARPA text file (repr() of the floats: they read back exactly).  The highest order carries no backoff
    column, a zero backoff below it is written out all the same."""
    by = {k: sorted(g for g in entries if len(g) == k) for k in range(1, order + 1)}
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for k in range(1, order + 1):
            f.write("ngram %d=%d\n" % (k, len(by[k])))
        for k in range(1, order + 1):
            f.write("\n\\%d-grams:\n" % k)
            for g in by[k]:
                logp, bo = entries[g]
                f.write("%r\t%s%s\n" % (float(logp), " ".join(g), "\t%r" % float(bo) if k < order else ""))
        f.write("\n\\end\\\n")
