"""Ragged sentence corpora for the CBOW trainer (n2v_hip/cbow.py, csrc/n2v_cbow.hip): a CSR pair ``tokens`` /
``offsets`` on the device instead of the fixed-stride walk matrix, so that playlists of 2 ... thousands of tracks
cost no padding.

``SentenceCorpus.from_sentences`` restates what gensim 3.2.0's ``build_vocab`` does before training
(src/extract_playlist.py:31-34: ``Word2Vec(sentences, min_count=min_ct)``): words rarer than ``min_count`` vanish from
their sentences before any window is cut, the kept words are indexed by descending count.  Two choices gensim leaves
open or makes differently are fixed here:
  * ties in count are broken by ascending ``np.unique`` order of the labels (gensim: whatever order its dict yields);
  * a sentence of more than MAX_SENTENCE = 4096 kept tokens is cut into consecutive sentences (gensim cuts at 10 000
    raw tokens): 4096 is what one wavefront's LDS slot holds.
Sentences that pruning empties stay as empty rows, so sentence ids (which key the random streams) do not shift.
"""
import numpy as np
import torch

from . import _lib

MAX_SENTENCE = 4096   # n2v_cbow_max_sentence()
CORPUS_BAD = [(1, "offsets do not start at 0"), (2, "the last offset is not the token count"),
              (4, "offsets decrease"), (8, "a sentence is longer than max_len"),
              (16, "a token is >= n_words")]   # N2V_CBOW_BAD_* of include/n2v_hip.h


def _device(device):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("n2v_hip: no GPU visible; there is no CPU fallback")
    return torch.device("cuda:%d" % torch.cuda.current_device())


def cut_offsets(offsets, max_len=MAX_SENTENCE):
    """offsets int64[S + 1] (device) -> offsets in which every sentence longer than max_len is replaced by consecutive
    sentences of max_len tokens (the last one shorter); shorter ones, empty ones included, stay one row each."""
    lens = offsets[1:] - offsets[:-1]
    pieces = torch.clamp((lens + (max_len - 1)) // max_len, min=1)
    if int(pieces.numel()) == 0 or int(pieces.max().item()) == 1:
        return offsets
    first = torch.cumsum(pieces, 0) - pieces
    owner = torch.repeat_interleave(torch.arange(lens.numel(), device=offsets.device), pieces)
    j = torch.arange(owner.numel(), device=offsets.device) - first[owner]
    return torch.cat([offsets[:-1][owner] + j * max_len, offsets[-1:]])


class SentenceCorpus:
    """tokens int32[T] and offsets int64[S + 1] on the device (sentence s = tokens[offsets[s]:offsets[s+1]], tokens < 0
    are padding); labels: dense id -> label (host); counts int64[N] (host): occurrences of each id in `tokens`;
    max_len: the longest sentence, at least 1."""

    def __init__(self, tokens, offsets, labels, counts, max_len):
        assert tokens.dtype == torch.int32 and offsets.dtype == torch.int64 and tokens.device == offsets.device
        self.tokens, self.offsets = tokens.contiguous(), offsets.contiguous()
        self.labels, self.counts, self.max_len = labels, np.asarray(counts, dtype=np.int64), int(max_len)
        self._checked = None

    @property
    def device(self):
        return self.tokens.device

    @property
    def n_sentences(self):
        return int(self.offsets.numel()) - 1

    @property
    def n_tokens(self):
        return int(self.tokens.numel())

    def __len__(self):
        return self.n_sentences

    @classmethod
    def from_sentences(cls, sentences, min_count=5, device=None):
        """sentences: any iterable of lists of hashable, mutually comparable labels (track ids, words)."""
        dev = _device(device)
        rows = [list(s) for s in sentences]
        lens = np.fromiter((len(r) for r in rows), dtype=np.int64, count=len(rows))
        flat = [w for r in rows for w in r]
        if flat:
            uniq, inverse = np.unique(np.asarray(flat), return_inverse=True)
        else:
            uniq, inverse = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        raw_off = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum(lens, out=raw_off[1:])
        ids = torch.from_numpy(inverse.astype(np.int64).reshape(-1)).to(dev)
        return cls.from_ids(uniq, ids, torch.from_numpy(raw_off).to(dev), min_count)

    @classmethod
    def from_ids(cls, uniq, ids, off, min_count=5):
        """ids int64[T] (device): positions in `uniq` (host, np.unique order); off int64[S + 1] (device).  Counting,
        pruning, remapping and compaction: torch ops on the device."""
        min_count = int(min_count)
        if min_count < 0:
            raise ValueError("min_count must be >= 0")
        dev = ids.device
        cnt = torch.bincount(ids, minlength=len(uniq))
        order = torch.sort(cnt, descending=True, stable=True).indices       # ties: ascending np.unique position
        order = order[cnt[order] >= max(min_count, 1)]
        remap = torch.full((len(uniq),), -1, dtype=torch.int64, device=dev)
        remap[order] = torch.arange(order.numel(), device=dev)
        new = remap[ids]
        kept = new >= 0
        before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(kept.long(), 0)])
        offsets = cut_offsets(before[off])
        tokens = new[kept].to(torch.int32)
        slen = offsets[1:] - offsets[:-1]
        max_len = max(1, int(slen.max().item())) if slen.numel() else 1
        labels = np.asarray(uniq)[order.cpu().numpy()]
        return cls(tokens, offsets, labels, cnt[order].cpu().numpy(), max_len)

    @classmethod
    def from_walks(cls, walks):
        """The walk matrix of a node2vec.WalkCorpus (int32 [W, L], -1 padded) seen as W sentences of L tokens: no copy
        (the padding is dropped by the kernel, token positions are the matrix columns as in the skip-gram trainer)."""
        w = walks.walks
        W, L = int(w.shape[0]), int(w.shape[1])
        if L > MAX_SENTENCE:
            raise ValueError("walks of %d nodes exceed the %d tokens a sentence may hold" % (L, MAX_SENTENCE))
        assert w.dtype == torch.int32 and w.is_contiguous()
        tokens = w.reshape(-1)
        offsets = torch.arange(W + 1, dtype=torch.int64, device=w.device) * L
        flat = tokens[tokens >= 0].long()
        counts = torch.bincount(flat, minlength=len(walks.labels)).cpu().numpy()
        return cls(tokens, offsets, walks.labels, counts, max(L, 1))

    def check(self, n_words):
        """n2v_cbow_corpus_check: a malformed corpus is a ValueError that names the cause (one read-back of an int32)
        and never reaches the training kernel."""
        n_words = int(n_words)
        if self._checked == n_words:
            return self
        if self.tokens.device.type != "cuda":
            raise RuntimeError("n2v_hip: the corpus is not on a GPU; there is no CPU fallback")
        if self.offsets.numel() < 1:
            raise ValueError("malformed corpus: offsets is empty")
        if not 1 <= self.max_len <= MAX_SENTENCE:
            raise ValueError("malformed corpus: max_len %d outside [1, %d]" % (self.max_len, MAX_SENTENCE))
        lib = _lib.load()
        dev = self.tokens.device
        with torch.cuda.device(dev):
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(lib.n2v_cbow_corpus_check(_lib.ptr(self.tokens), _lib.ptr(self.offsets), self.n_sentences,
                                                 self.n_tokens, n_words, self.max_len, _lib.ptr(status),
                                                 _lib.stream_ptr(dev)))
            bits = int(status.item())
        if bits:
            raise ValueError("malformed corpus: " + "; ".join(msg for b, msg in CORPUS_BAD if bits & b))
        self._checked = n_words
        return self

    def tolist(self):
        """Sentences of labels (host), padding dropped."""
        t, o = self.tokens.cpu().numpy(), self.offsets.cpu().numpy()
        lab = self.labels
        return [[lab[x].item() if hasattr(lab[x], "item") else lab[x] for x in t[o[s]:o[s + 1]] if x >= 0]
                for s in range(len(o) - 1)]
