"""Host side of the CBOW / negative-sampling trainer (gensim's ``Word2Vec(sentences, sg=0)``, what
src/extract_playlist.py:31-34 trains as song2vec) on MI355X: vocabulary statistics and the schedule are prepared
here, every row update runs in the HIP kernel ``n2v_cbow_train`` (csrc/n2v_cbow.hip) over a ragged
``SentenceCorpus`` (n2v_hip/corpus.py).

gensim 3.2.0 is a third-party dependency that is not part of the reference tree: the update rule is
restated from memory in csrc/n2v_cbow.hip (tests/cbow_reference.py is its float64 restatement) and parity with gensim
is UNPINNED.  The tables, their initialisation, the cum-table and sub-sampling thresholds and the job-wise learning
rate are the skip-gram trainer's (n2v_hip/sgns.py); the sub-sampling threshold uses the total of the RETAINED counts,
the words that survived ``min_count``.  Rows are changed by float atomic adds only (no lossy mode), on one GPU.
"""
import numpy as np
import torch

from . import _lib
from . import sgns as _sgns
from .corpus import SentenceCorpus

UPDATE_MODE = _sgns.UPDATE_MODES["atomic"]   # the only mode n2v_cbow_train accepts


class RaggedModel:
    """Embedding tables + vocabulary statistics of one training run over a SentenceCorpus, on one device: what the CBOW
    trainer and the skip-gram trainer (n2v_hip/skipgram.py) share."""

    def __init__(self, n_words, dim=100, window=5, negative=5, alpha=0.025, min_alpha=1e-4, sample=1e-3, seed=1,
                 device=None, what="CBOW"):
        if not torch.cuda.is_available():
            raise RuntimeError("n2v_hip: no GPU visible; the %s trainer has no CPU fallback" % what)
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.n_words, self.dim = int(n_words), int(dim)
        self.stride = _sgns._row_stride(self.dim)
        self.window, self.negative = int(window), int(negative)
        self.alpha, self.min_alpha, self.sample, self.seed = float(alpha), float(min_alpha), sample, int(seed)
        d = self.device
        self.syn0 = torch.empty((self.n_words, self.stride), dtype=torch.float32, device=d)
        self.syn1neg = torch.empty((self.n_words, self.stride), dtype=torch.float32, device=d)
        self.pair_count = torch.zeros(1, dtype=torch.int64, device=d)     # trained centres (CBOW) / pairs (skip-gram)
        self.work_counter = torch.zeros(1, dtype=torch.int64, device=d)   # in-order hand-out; None: static grid stride
        self.counts = None
        self.sample_int = self.cum_table = self.lut = None
        self.reset_weights()

    def _stream(self):
        return _lib.stream_ptr(self.device)

    def reset_weights(self):
        with torch.cuda.device(self.device):
            _lib.check(self.lib.n2v_sgns_init(_lib.ptr(self.syn0), _lib.ptr(self.syn1neg), self.n_words, self.dim,
                                              self.stride, self.seed & (2**64 - 1), self._stream()))

    def build_vocab(self, counts):
        """counts int64[n_words]: occurrences of each id among the RETAINED tokens (SentenceCorpus.counts)."""
        counts = np.asarray(counts, dtype=np.int64)
        if counts.shape != (self.n_words,):
            raise ValueError("counts must hold one entry per word")
        d = self.device
        self.counts = counts
        sample_int, cum = _sgns.vocab_tables(counts, self.sample)
        self.sample_int = None if sample_int is None else torch.from_numpy(sample_int.view(np.int32)).to(d)
        self.cum_table = torch.from_numpy(cum.view(np.int32)).to(d)
        self.lut = torch.empty((1 << _sgns.LUT_BITS) + 1, dtype=torch.int32, device=d)
        with torch.cuda.device(d):
            _lib.check(self.lib.n2v_build_neg_lut(_lib.ptr(self.cum_table), self.n_words, _sgns.LUT_BITS,
                                                  _lib.ptr(self.lut), self._stream()))

    def _check_corpus(self, corpus):
        if not isinstance(corpus, SentenceCorpus):
            raise TypeError("train_pass takes a SentenceCorpus")
        if self.cum_table is None:
            raise RuntimeError("build_vocab first")
        if corpus.device != self.device:
            raise ValueError("corpus on %s, model on %s" % (corpus.device, self.device))
        corpus.check(self.n_words)

    def pairs_trained(self):
        """Centres trained so far (a centre without context trains nothing and is not counted)."""
        return int(self.pair_count.item())

    def vectors(self):
        """syn0 without the padding columns (device view)."""
        return self.syn0[:, :self.dim]


class CbowModel(RaggedModel):
    """Embedding tables + vocabulary statistics of one CBOW training run, on one device."""

    def __init__(self, n_words, dim=100, window=5, negative=5, cbow_mean=1, alpha=0.025, min_alpha=1e-4, sample=1e-3,
                 seed=1, device=None):
        if int(n_words) < 1:
            raise ValueError("empty vocabulary")
        if int(window) < 1 or not 0 <= int(negative) <= 64 or cbow_mean not in (0, 1, False, True):
            raise ValueError("window must be >= 1, negative in [0, 64], cbow_mean 0 or 1")
        self.cbow_mean = int(bool(cbow_mean))
        RaggedModel.__init__(self, n_words, dim=dim, window=window, negative=negative, alpha=alpha, min_alpha=min_alpha,
                             sample=sample, seed=seed, device=device, what="CBOW")

    def train_pass(self, corpus, sentences_base, sentences_total, sentence_id_base, sentences_step=1, alpha_batch=None,
                   max_blocks=0, first=0, count=None):
        """One kernel launch over the corpus (or its sentences [first, first + count): the launch then numbers them
        from 0); asynchronous.  The corpus is checked (once, as a whole) before anything is launched."""
        self._check_corpus(corpus)
        first = int(first)
        count = corpus.n_sentences - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > corpus.n_sentences:
            raise ValueError("sentences [%d, %d) outside the corpus" % (first, first + count))
        if count == 0 or corpus.n_tokens == 0:
            return
        if alpha_batch is None:
            alpha_batch = default_alpha_batch(corpus)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.n2v_cbow_train(
                _lib.ptr(corpus.tokens), _lib.ptr(corpus.offsets) + 8 * first, count, corpus.n_tokens, corpus.max_len,
                _lib.ptr(self.syn0), _lib.ptr(self.syn1neg), self.n_words, self.dim, self.stride, self.window,
                self.negative, self.cbow_mean, _lib.ptr(self.sample_int), _lib.ptr(self.cum_table), _lib.ptr(self.lut),
                _sgns.LUT_BITS, self.alpha, self.min_alpha, int(sentences_base), int(sentences_step),
                int(sentences_total), int(alpha_batch), self.seed & (2**64 - 1), int(sentence_id_base) & (2**64 - 1),
                _lib.ptr(self.pair_count), UPDATE_MODE, int(max_blocks), _lib.ptr(self.work_counter), self._stream()))


def default_alpha_batch(corpus):
    """Sentences per learning-rate step: gensim steps alpha once per job of <= 10 000 words."""
    if corpus.n_sentences == 0 or corpus.n_tokens == 0:
        return 1
    return max(1, int(round(_sgns.MAX_WORDS_IN_BATCH / (corpus.n_tokens / corpus.n_sentences))))


def train(model, corpus, epochs=5, max_blocks=0, sequential=False):
    """`epochs` passes over the corpus; epoch e uses the sentence ids e * S + s and the learning rate runs linearly
    over all epochs * S sentences.  sequential=True launches the sentences one after the other, each on one wavefront
    (gensim's workers=1): the same schedule, ids and draws, and a result that is reproducible to the bit — for tests and
    small corpora, a launch per sentence is slow."""
    S = corpus.n_sentences
    if S == 0:
        return
    batch = default_alpha_batch(corpus)
    if sequential:
        lens = (corpus.offsets[1:] - corpus.offsets[:-1]).cpu().numpy()
        for ep in range(int(epochs)):
            for s in np.nonzero(lens > 1)[0].tolist():       # a sentence of one word trains nothing
                model.train_pass(corpus, sentences_base=ep * S + (s // batch) * batch, sentences_total=int(epochs) * S,
                                 sentence_id_base=ep * S + s, alpha_batch=batch, max_blocks=1, first=s, count=1)
        return
    for ep in range(int(epochs)):
        model.train_pass(corpus, sentences_base=ep * S, sentences_total=int(epochs) * S, sentence_id_base=ep * S,
                         alpha_batch=batch, max_blocks=max_blocks)
