"""``Word2Vec(sentences, ...)`` with gensim 3.2.0's argument names and defaults, trained on the GPU: what
src/extract_playlist.py:31-34 calls as ``gensim.models.Word2Vec(sentences, min_count=min_ct)`` (CBOW: sg=0,
cbow_mean=1, size 100, window 5, 5 negatives, iter 5).  Returns the ``Word2VecResult`` / ``KeyedVectors`` pair of
n2v_hip/sgns.py, keyed by the sentences' own labels.  ``Word2Vec(..., sg=1)`` still refuses (its callers rely on the
refusal); skip-gram over ragged sentences is ``SkipGram(sentences, ...)`` below (n2v_hip/skipgram.py,
csrc/n2v_sgns_csr.hip)."""
import numpy as np

from . import cbow as _cbow
from . import sgns as _sgns
from . import skipgram as _skipgram
from .corpus import SentenceCorpus


class LabelKeyedVectors(_sgns.KeyedVectors):
    """KeyedVectors over arbitrary hashable labels; `labels` / `counts` / `vectors` come sorted by descending count
    (SentenceCorpus order)."""

    def __init__(self, labels, counts, vectors):
        self.index2word = [x.item() if hasattr(x, "item") else x for x in labels]
        self.syn0 = np.ascontiguousarray(vectors, dtype=np.float32)
        self.vectors = self.syn0
        self.vocab = {w: _sgns._VocabEntry(i, int(counts[i])) for i, w in enumerate(self.index2word)}
        self.vector_size = self.syn0.shape[1] if self.syn0.ndim == 2 else 0


def _train_ragged(sentences, size, min_count, iter, device, make_model, train, own_checks=None):
    """What Word2Vec and SkipGram below share: the size / iter checks, then the caller's own (in its order of refusal),
    the corpus, `make_model(corpus)`, `train(model, corpus)` and the result keyed by the sentences' labels."""
    if int(size) < 1 or int(size) > 512:
        raise ValueError("size must be in [1, 512]")
    if int(iter) < 1:
        raise ValueError("iter must be >= 1")
    if own_checks is not None:
        own_checks()
    corpus = sentences if isinstance(sentences, SentenceCorpus) else SentenceCorpus.from_sentences(
        sentences, min_count=min_count, device=device)
    if len(corpus.labels) == 0:
        raise ValueError("no word occurs min_count=%d times: the vocabulary is empty" % int(min_count))
    model = make_model(corpus)
    model.build_vocab(corpus.counts)
    train(model, corpus)
    wv = LabelKeyedVectors(corpus.labels, corpus.counts, model.vectors().cpu().numpy())
    return _sgns.Word2VecResult(wv, model, model.pairs_trained())


def Word2Vec(sentences, size=100, window=5, min_count=5, sg=0, negative=5, cbow_mean=1, alpha=0.025, min_alpha=1e-4,
             sample=1e-3, iter=5, seed=1, device=None, sequential=False):
    """sentences: an iterable of lists of labels, or a SentenceCorpus (then min_count has been applied already).
    sequential=True: one sentence at a time on one wavefront, reproducible to the bit (n2v_hip/cbow.py:train).
    sg=1 is refused here: skip-gram over ragged sentences is SkipGram(sentences, ...)."""
    if sg not in (0, 1):
        raise ValueError("sg must be 0 (CBOW) or 1 (skip-gram)")
    if sg == 1:
        raise NotImplementedError("sg=1 over ragged sentences is not built; main.learn_embeddings trains skip-gram "
                                  "on a walk matrix")
    return _train_ragged(
        sentences, size, min_count, iter, device,
        lambda corpus: _cbow.CbowModel(len(corpus.labels), dim=size, window=window, negative=negative, cbow_mean=cbow_mean,
                                       alpha=alpha, min_alpha=min_alpha, sample=sample, seed=seed, device=corpus.device),
        lambda model, corpus: _cbow.train(model, corpus, epochs=iter, sequential=sequential))


def SkipGram(sentences, size=100, window=5, min_count=5, negative=5, alpha=0.025, min_alpha=1e-4, sample=1e-3, iter=5,
             seed=1, device=None, sequential=False, chunk="auto"):
    """gensim's Word2Vec(sentences, sg=1, ...) over ragged sentences: same arguments, corpus and result as Word2Vec
    above.  chunk: centres per work item ("auto": whole sentences up to 256 tokens, else 256; 0: whole sentences);
    sequential=True: one item at a time on one wavefront, reproducible to the bit (n2v_hip/skipgram.py:train)."""
    def own_checks():
        _sgns.check_window_negative(window, negative)
        if not (chunk == "auto" or (isinstance(chunk, (int, np.integer)) and not isinstance(chunk, bool) and chunk >= 0)):
            raise ValueError("chunk must be 'auto' or an int >= 0")
        if chunk != "auto" and ((int(chunk) + 2 * int(window) + 63) // 64) * 64 > _skipgram.MAX_SLOT:
            raise ValueError("chunk %d + 2 x window %d exceeds the %d tokens a wavefront stages" % (chunk, window, _skipgram.MAX_SLOT))

    return _train_ragged(
        sentences, size, min_count, iter, device,
        lambda corpus: _skipgram.SkipGramModel(len(corpus.labels), dim=size, window=window, negative=negative, alpha=alpha,
                                               min_alpha=min_alpha, sample=sample, seed=seed, device=corpus.device),
        lambda model, corpus: _skipgram.train(model, corpus, epochs=iter, chunk=chunk, sequential=sequential),
        own_checks)
