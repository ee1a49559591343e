"""Host side of the CBOW / negative-sampling trainer (gensim's ``Word2Vec(sentences, sg=0)``, what
src/extract_playlist.py:31-34 trains as song2vec) on MI355X: vocabulary statistics and the schedule are prepared
here, every row update runs in the HIP kernel ``n2v_cbow_train`` (csrc/n2v_cbow.hip) over a ragged
``SentenceCorpus`` (n2v_hip/corpus.py).

gensim 3.2.0 is a third-party dependency that is not part of the reference tree: the update rule is
restated from memory in csrc/n2v_cbow.hip (tests/cbow_reference.py is its float64 restatement) and parity with gensim
is UNPINNED.  ``RaggedModel`` below owns the tables of both trainers over ragged sentences; the tables' layout, their
initialisation, the cum-table and sub-sampling thresholds and the job-wise learning rate are the skip-gram trainer's
(n2v_hip/sgns.py: ``W2vTables``); the sub-sampling threshold uses the total of the RETAINED counts, the words that
survived ``min_count``.  Rows are changed by float atomic adds only (no lossy mode), on one GPU.
"""
import numpy as np
import torch

from . import _lib
from . import sgns as _sgns
from .corpus import SentenceCorpus

UPDATE_MODE = _sgns.UPDATE_MODES["atomic"]   # the only mode n2v_cbow_train accepts


class RaggedModel(_sgns.W2vTables):
    """Embedding tables + vocabulary statistics of one training run over a SentenceCorpus, on one device: what the CBOW
    trainer and the skip-gram trainer (n2v_hip/skipgram.py) share.  The tables, their initialisation and the upload of
    the statistics are sgns.W2vTables'; pair_count holds trained centres (CBOW) or pairs (skip-gram)."""

    def __init__(self, n_words, dim=100, window=5, negative=5, alpha=0.025, min_alpha=1e-4, sample=1e-3, seed=1,
                 device=None, what="CBOW"):
        _sgns.W2vTables.__init__(self, what, n_words, dim, window, negative, alpha, min_alpha, sample, seed, device)

    def build_vocab(self, counts):
        """counts int64[n_words]: occurrences of each id among the RETAINED tokens (SentenceCorpus.counts)."""
        counts = np.asarray(counts, dtype=np.int64)
        if counts.shape != (self.n_words,):
            raise ValueError("counts must hold one entry per word")
        self._set_vocab(counts)

    def _check_corpus(self, corpus):
        if not isinstance(corpus, SentenceCorpus):
            raise TypeError("train_pass takes a SentenceCorpus")
        if self.cum_table is None:
            raise RuntimeError("build_vocab first")
        if corpus.device != self.device:
            raise ValueError("corpus on %s, model on %s" % (corpus.device, self.device))
        corpus.check(self.n_words)


class CbowModel(RaggedModel):
    """Embedding tables + vocabulary statistics of one CBOW training run, on one device."""

    def __init__(self, n_words, dim=100, window=5, negative=5, cbow_mean=1, alpha=0.025, min_alpha=1e-4, sample=1e-3,
                 seed=1, device=None):
        if int(n_words) < 1:
            raise ValueError("empty vocabulary")
        _sgns.check_window_negative(window, negative)
        if cbow_mean not in (0, 1, False, True):
            raise ValueError("cbow_mean must be 0 or 1")
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
        tables = self._tables()         # n2v_cbow_train takes cbow_mean between `negative` and `sample_int`
        with torch.cuda.device(self.device):
            _lib.check(self.lib.n2v_cbow_train(
                _lib.ptr(corpus.tokens), _lib.ptr(corpus.offsets) + 8 * first, count, corpus.n_tokens, corpus.max_len,
                *tables[:7], self.cbow_mean, *tables[7:], int(sentences_base), int(sentences_step), int(sentences_total),
                int(alpha_batch), self._seed64(), int(sentence_id_base) & (2**64 - 1), _lib.ptr(self.pair_count),
                UPDATE_MODE, int(max_blocks), _lib.ptr(self.work_counter), self._stream()))


def default_alpha_batch(corpus):
    """Sentences per learning-rate step: gensim steps alpha once per job of <= 10 000 words."""
    if corpus.n_sentences == 0 or corpus.n_tokens == 0:
        return 1
    return max(1, int(round(_sgns.MAX_WORDS_IN_BATCH / (corpus.n_tokens / corpus.n_sentences))))


def trainable_sentences(corpus):
    """The sentences a sequential pass launches, in order: a sentence of one word (or none) trains nothing."""
    lens = (corpus.offsets[1:] - corpus.offsets[:-1]).cpu().numpy()
    return np.nonzero(lens > 1)[0].tolist()


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
        todo = trainable_sentences(corpus)
        for ep in range(int(epochs)):
            for s in todo:
                model.train_pass(corpus, sentences_base=ep * S + (s // batch) * batch, sentences_total=int(epochs) * S,
                                 sentence_id_base=ep * S + s, alpha_batch=batch, max_blocks=1, first=s, count=1)
        return
    for ep in range(int(epochs)):
        model.train_pass(corpus, sentences_base=ep * S, sentences_total=int(epochs) * S, sentence_id_base=ep * S,
                         alpha_batch=batch, max_blocks=max_blocks)
