"""Host side of the skip-gram / negative-sampling trainer over a ragged ``SentenceCorpus`` (gensim's
``Word2Vec(sentences, sg=1)``) on MI355X: every row update runs in the HIP kernel ``n2v_sgns_csr_train``
(csrc/n2v_sgns_csr.hip).  ``RaggedModel`` (n2v_hip/cbow.py) owns the tables and the vocabulary statistics, and the
schedule is the CBOW trainer's; the update rule per (centre, context) pair is the walk-matrix trainer's
(csrc/n2v_sgns.hip), so a -1-padded walk matrix seen through ``SentenceCorpus.from_walks`` trains the same streams.
Parity with gensim is UNPINNED, as for both of those.  Rows are changed by float atomic adds only, on one GPU.

Work items: with ``chunk == 0`` a sentence is one item on one wavefront.  With ``chunk >= 1`` sentence s of n_s raw
tokens is dealt to ``ceil(n_s / chunk)`` items of at most ``chunk`` centres each; a wavefront's LDS slot is then
``chunk + 2 * window`` tokens instead of the corpus' longest sentence, and no item is longer than ``chunk`` centres.
"""
import torch

from . import _lib
from . import cbow as _cbow
from . import sgns as _sgns
from .cbow import default_alpha_batch
from .corpus import SentenceCorpus

UPDATE_MODE = _sgns.UPDATE_MODES["atomic"]   # the only mode n2v_sgns_csr_train accepts
MAX_SLOT = 4096                              # tokens of a wavefront's LDS slot
AUTO_CHUNK = 256                             # provisional: ~1 500 pairs (~4 ms of one wave) per item, 5 KiB of LDS per workgroup
AUTO_CHUNK_MIN_LEN = 256                     # corpora whose longest sentence is at most this long are not chunked


def resolve_chunk(corpus, chunk):
    """"auto" -> 0 (whole sentences) when corpus.max_len <= 256, else 256; an int >= 0 is taken as it is."""
    if isinstance(chunk, str):
        if chunk != "auto":
            raise ValueError("chunk must be 'auto' or an int >= 0")
        return 0 if corpus.max_len <= AUTO_CHUNK_MIN_LEN else AUTO_CHUNK
    chunk = int(chunk)
    if chunk < 0:
        raise ValueError("chunk must be 'auto' or an int >= 0")
    return chunk


def _items(corpus, chunk):
    """(item_off tensor or None, number of items), cached on the corpus per chunk."""
    chunk = int(chunk)
    if chunk < 0:
        raise ValueError("chunk must be >= 0")
    if chunk == 0:
        return None, corpus.n_sentences
    cache = corpus.__dict__.setdefault("_item_offsets", {})
    if chunk not in cache:
        lens = corpus.offsets[1:] - corpus.offsets[:-1]
        per = (lens + (chunk - 1)) // chunk                    # ceil(n_s / chunk), 0 for an empty sentence
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=corpus.offsets.device), torch.cumsum(per, 0)])
        cache[chunk] = (off.contiguous(), int(off[-1].item()))
    return cache[chunk]


def item_offsets(corpus, chunk):
    """int64[S + 1] on the corpus' device: item_off[s] = first item of sentence s, item_off[S] = the item count
    (sentence s has ceil(n_s / chunk) items).  None with chunk == 0: an item is a sentence."""
    return _items(corpus, chunk)[0]


def n_items(corpus, chunk):
    """Items of the corpus at this chunk (the sentence count with chunk == 0)."""
    return _items(corpus, chunk)[1]


class SkipGramModel(_cbow.RaggedModel):
    """Embedding tables + vocabulary statistics of one skip-gram training run over a SentenceCorpus, on one device."""

    def __init__(self, n_words, dim=100, window=5, negative=5, alpha=0.025, min_alpha=1e-4, sample=1e-3, seed=1,
                 device=None):
        if int(n_words) < 1:
            raise ValueError("empty vocabulary")
        _sgns.check_window_negative(window, negative)
        _cbow.RaggedModel.__init__(self, n_words, dim=dim, window=window, negative=negative, alpha=alpha,
                                   min_alpha=min_alpha, sample=sample, seed=seed, device=device, what="skip-gram")

    def train_pass(self, corpus, sentences_base, sentences_total, sentence_id_base, sentences_step=1, alpha_batch=None,
                   chunk=0, first_item=0, item_count=None, max_blocks=0):
        """One kernel launch over the items [first_item, first_item + item_count) of the corpus (default: all);
        asynchronous.  Sentence s has id sentence_id_base + s and the learning rate of job s // alpha_batch, whichever
        items are launched.  The corpus is checked (once, as a whole) before anything is launched."""
        self._check_corpus(corpus)
        chunk = int(chunk)
        item_off, total = _items(corpus, chunk)
        first_item = int(first_item)
        n_items = total - first_item if item_count is None else int(item_count)
        if first_item < 0 or n_items < 0 or first_item + n_items > total:
            raise ValueError("items [%d, %d) outside the corpus' %d items (chunk %d)"
                             % (first_item, first_item + n_items, total, chunk))
        if n_items == 0 or corpus.n_tokens == 0:
            return
        if alpha_batch is None:
            alpha_batch = default_alpha_batch(corpus)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.n2v_sgns_csr_train(
                _lib.ptr(corpus.tokens), _lib.ptr(corpus.offsets), corpus.n_sentences, corpus.n_tokens, corpus.max_len,
                _lib.ptr(item_off), chunk, first_item, n_items, *self._tables(), int(sentences_base),
                int(sentences_step), int(sentences_total), int(alpha_batch), self._seed64(),
                int(sentence_id_base) & (2**64 - 1), _lib.ptr(self.pair_count), UPDATE_MODE, int(max_blocks),
                _lib.ptr(self.work_counter), self._stream()))


def train(model, corpus, epochs=5, chunk="auto", sequential=False, max_blocks=0):
    """`epochs` passes over the corpus with cbow.train's schedule: epoch e uses the sentence ids e * S + s and the
    learning rate runs linearly over all epochs * S sentences.  sequential=True launches the items one after the other,
    each on one wavefront: the same schedule, ids and draws, and a result that is reproducible to the bit — for tests
    and small corpora, a launch per item is slow."""
    if not isinstance(corpus, SentenceCorpus):
        raise TypeError("train takes a SentenceCorpus")
    S = corpus.n_sentences
    if S == 0:
        return
    chunk = resolve_chunk(corpus, chunk)
    batch = default_alpha_batch(corpus)
    for ep in range(int(epochs)):
        kw = dict(sentences_base=ep * S, sentences_total=int(epochs) * S, sentence_id_base=ep * S, alpha_batch=batch,
                  chunk=chunk)
        if not sequential:
            model.train_pass(corpus, max_blocks=max_blocks, **kw)
            continue
        todo = _cbow.trainable_sentences(corpus) if chunk == 0 else range(n_items(corpus, chunk))
        for item in todo:
            model.train_pass(corpus, first_item=item, item_count=1, max_blocks=1, **kw)
