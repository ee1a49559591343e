"""Host tests of the ragged skip-gram trainer (n2v_hip/skipgram.py, word2vec.SkipGram, extract_playlist -sg;
csrc/n2v_sgns_csr.hip): what can be checked without a GPU.

(a) the chunked decomposition is exact: tests/sgcsr_reference.py trained item by item, in order, equals
    tests/sgns_reference.py on the whole sentence bit for bit in float64, pairs included;
(b) `item_offsets` equals a brute-force loop, and no item holds more than `chunk` centres;
(c) the errors the chunked design invites, planted in the restatement, against the GPU tolerance TOL = 1e-5 on a corpus
    chosen here so that they show (chunk 4, window 5, sub-sampling and -1 tokens, a learning-rate step per sentence).
    Measured, as the largest relative deviation of a table: context clipped at the chunk border 4.5e-1, skip by
    pairs_before without `* negative` 1.3e-1, alpha per item instead of per sentence 1.7e-1: each >= 12 000 x TOL.
    Split bounds from the raw rather than the effective length are NOT observable in the tables: the bounds only
    partition the centres [0, n_eff) among the items, and any monotone partition (clipped to n_eff) trains the same
    pairs in the same order with the same draws — what it costs is balance (the last items of a sub-sampled sentence are
    empty), not values.  Its deviation is asserted to be exactly 0 rather than dropped.  Likewise alpha per item where
    every sentence is one item (chunk 0) and the skip without `* negative` at negative == 1 are asserted to be exactly 0;
(d) no sigmoid evaluation of the GPU case table sits near a bin edge (a condition of the data, not of the kernel);
(e) the C-ABI; (f) argument errors; (g) the kernel compiles for gfx950 without scratch.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sgcsr_cases as K
import sgcsr_reference as G
import sgns_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "node2vec-by-ecc_amd", "csrc")


def _tables(rs, n, dim):
    return rs.random_sample((n, dim)) - 0.5, rs.random_sample((n, dim)) - 0.5


def _kw(counts, sample, **over):
    sample_int, cum = K.vocab(counts, sample)
    kw = dict(window=3, negative=2, alpha=0.05, min_alpha=1e-4, sample_int=sample_int, cum_table=cum, seed=2**40 + 3,
              sentence_id_base=17, sentences_base=3, sentences_step=2, sentences_total=400, alpha_batch=3)
    kw.update(over)
    return kw


# ---- (a) the decomposition ---------------------------------------------------------------------------------------------

def _whole_sentences(s0, s1, tokens, offsets, kw):
    """sgns_reference.train, one sentence at a time, with the job-wise schedule of the corpus."""
    stats = R.Stats()
    base = {k: v for k, v in kw.items() if k not in ("sentence_id_base", "sentences_base")}
    for s in range(len(offsets) - 1):
        raw = tokens[offsets[s]:offsets[s + 1]]
        pushed = kw["sentences_base"] + (s // kw["alpha_batch"]) * kw["alpha_batch"] * kw["sentences_step"]
        R.train(s0, s1, raw[None, :], None, walk_id_base=kw["sentence_id_base"] + s, sentences_base=pushed, stats=stats,
                **base)
    return stats


@pytest.mark.parametrize("chunk,window,sample,minus1,lens", [
    (1, 1, 0, False, range(0, 4)), (1, 3, 1e-2, False, list(range(0, 4)) + [300]),
    (2, 3, 0, True, list(range(0, 6)) + [300]), (2, 2, 1e-2, False, range(0, 6)),
    (3, 3, 1e-2, True, list(range(0, 8)) + [300]), (3, 7, 0, False, range(0, 8)),
    (64, 3, 1e-2, True, list(range(0, 130)) + [300]), (64, 70, 1e-2, False, [63, 64, 65, 129, 300]),
])
def test_items_in_order_are_the_whole_sentence_bit_for_bit(chunk, window, sample, minus1, lens):
    rs = np.random.RandomState(11 + chunk)
    n, dim = 40, 4
    counts = (rs.pareto(1.0, n) * 20).astype(np.int64) + 1
    counts[:3] = [3000, 2000, 1200]
    p = counts / counts.sum()
    sents = [rs.choice(n, size=L, p=0.5 * p + 0.5 / n).astype(np.int32) for L in lens]
    if minus1:
        for s in sents:
            s[rs.random_sample(len(s)) < 0.15] = -1
    tokens = np.concatenate(sents).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sents])]).astype(np.int64)
    kw = _kw(counts, sample, window=window, negative=1 if chunk == 64 else 2)
    s0, s1 = _tables(rs, n, dim)
    a0, a1, b0, b1 = s0.copy(), s1.copy(), s0.copy(), s1.copy()
    pairs, _ = G.train(a0, a1, tokens, offsets, chunk, **kw)
    whole = _whole_sentences(b0, b1, tokens, offsets, kw)
    assert pairs == whole.pairs > 0
    assert (a0 != s0).any() and (a1 != s1).any()
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
    if sample:
        kept = sum(len(R.effective_sentence(s, len(s), kw["sample_int"], kw["seed"], kw["sentence_id_base"] + k))
                   for k, s in enumerate(sents))
        assert kept < int((tokens >= 0).sum()), "sub-sampling dropped nothing"
    # and an item range is the same items: first half, then the rest
    c0, c1 = s0.copy(), s1.copy()
    total = len(G.item_table(offsets, chunk))
    st = R.Stats()
    G.train(c0, c1, tokens, offsets, chunk, first_item=0, n_items=total // 2, stats=st, **kw)
    G.train(c0, c1, tokens, offsets, chunk, first_item=total // 2, stats=st, **kw)
    assert st.pairs == pairs and np.array_equal(c0, a0) and np.array_equal(c1, a1)


# ---- (b) item_offsets --------------------------------------------------------------------------------------------------

def _cpu_corpus(lens, n_words=50, seed=0):
    import torch
    from n2v_hip.corpus import SentenceCorpus
    rs = np.random.RandomState(seed)
    lens = np.asarray(lens, np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tokens = rs.randint(0, n_words, int(lens.sum())).astype(np.int32)
    return SentenceCorpus(torch.from_numpy(tokens), torch.from_numpy(offsets), np.arange(n_words),
                          np.bincount(tokens, minlength=n_words), max(1, int(lens.max()) if len(lens) else 1))


@pytest.mark.parametrize("chunk", [0, 1, 2, 7, 64, 256])
def test_item_offsets_against_a_brute_force_loop(chunk):
    from n2v_hip import skipgram
    c = max(chunk, 1)
    lens = [0, 1, c - 1, c, c + 1, 0, 0, 2 * c - 1, 2 * c, 2 * c + 1, 5 * c + 3, 0, 4096, 1, 0]
    corpus = _cpu_corpus(lens)
    off = skipgram.item_offsets(corpus, chunk)
    table = G.item_table(corpus.offsets.numpy(), chunk)
    assert skipgram.n_items(corpus, chunk) == len(table)
    if chunk == 0:
        assert off is None and len(table) == len(lens)
        return
    want = [0]
    for n in lens:
        want.append(want[-1] + (n + chunk - 1) // chunk)
    assert off.dtype == __import__("torch").int64 and off.tolist() == want and want[-1] == len(table)
    assert skipgram.item_offsets(corpus, chunk) is off                       # cached per chunk
    assert skipgram.item_offsets(corpus, chunk + 1) is not off
    # every item maps back through the table, and holds at most `chunk` centres whatever sub-sampling leaves
    for item, (s, sp, S) in enumerate(table):
        assert want[s] + sp == item and S == want[s + 1] - want[s]
    for n in lens:
        S = (n + chunk - 1) // chunk
        for n_eff in {0, 1, n // 3, max(n - 1, 0), n}:
            bounds = [G.item_bounds(n_eff, sp, S) for sp in range(S)]
            assert all(e - b <= chunk for b, e in bounds)
            assert [b for b, _ in bounds][1:] == [e for _, e in bounds][:-1] and (not S or (bounds[0][0], bounds[-1][1]) == (0, n_eff))
    with pytest.raises(ValueError):
        skipgram.item_offsets(corpus, -1)


def test_auto_chunk():
    from n2v_hip import skipgram
    assert skipgram.resolve_chunk(_cpu_corpus([3, 256]), "auto") == 0
    assert skipgram.resolve_chunk(_cpu_corpus([3, 257]), "auto") == 256 == skipgram.AUTO_CHUNK
    assert skipgram.resolve_chunk(_cpu_corpus([3, 257]), 0) == 0 and skipgram.resolve_chunk(_cpu_corpus([3]), 64) == 64
    for bad in (-1, "big"):
        with pytest.raises(ValueError):
            skipgram.resolve_chunk(_cpu_corpus([3]), bad)


# ---- (c) planted errors ------------------------------------------------------------------------------------------------

def _planted_corpus():
    """chunk 4, window 5 (context crosses chunk borders on both sides), sub-sampling and -1 tokens (n_eff < n_s), three
    sentences of several items each with a learning-rate step per sentence."""
    rs = np.random.RandomState(5)
    n, dim = 60, 8
    counts = (rs.pareto(1.0, n) * 20).astype(np.int64) + 1
    counts[:3] = [3000, 2000, 1200]
    p = counts / counts.sum()
    sents = [rs.choice(n, size=L, p=0.5 * p + 0.5 / n).astype(np.int32) for L in (30, 0, 25, 41)]
    for s in sents:
        s[rs.random_sample(len(s)) < 0.1] = -1
    tokens = np.concatenate(sents).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sents])]).astype(np.int64)
    s0 = (rs.random_sample((n, dim)) - 0.5) / dim
    s1 = (rs.random_sample((n, dim)) - 0.5) * 0.2
    return counts, tokens, offsets, s0, s1


def _planted_run(variant, chunk=4, **over):
    counts, tokens, offsets, s0, s1 = _planted_corpus()
    kw = _kw(counts, 1e-2, **dict(dict(window=5, negative=3, alpha=0.025, sentences_base=0, sentences_step=1,
                                       sentences_total=40, alpha_batch=1), **over))
    a0, a1 = s0.copy(), s1.copy()
    G.train(a0, a1, tokens, offsets, chunk, variant=variant, **kw)
    return a0, a1


def test_every_planted_error_is_far_outside_the_gpu_tolerance():
    r0, r1 = _planted_run(None)
    moved = {}
    for v in G.VARIANTS:
        a0, a1 = _planted_run(v)
        moved[v] = max(K.relative_deviation(a0, a1, r0, r1))
        print("planted %-22s largest relative deviation %.3g = %.0f x TOL" % (v, moved[v], moved[v] / K.TOL))
    assert moved.pop("raw_split_bounds") == 0.0      # a partition of the centres, not an error of the tables (see above)
    assert len(moved) == 3 and min(moved.values()) > 1000 * K.TOL, moved
    # where an error cannot show, it shows exactly nothing: one item per sentence has the item's number equal to no
    # sentence's only by the empty sentence (chunk 0: items ARE sentences), and one draw per pair makes both skips equal
    w0, w1 = _planted_run(None, chunk=0)
    a0, a1 = _planted_run("alpha_per_item", chunk=0)
    assert max(K.relative_deviation(a0, a1, w0, w1)) == 0.0
    n0, n1 = _planted_run(None, negative=1)
    a0, a1 = _planted_run("skip_without_negative", negative=1)
    assert max(K.relative_deviation(a0, a1, n0, n1)) == 0.0
    # and chunking itself changes nothing
    assert np.array_equal(w0, r0) and np.array_equal(w1, r1)


# ---- (d) the GPU case table --------------------------------------------------------------------------------------------

def test_case_table_has_no_evaluation_on_a_bin_edge_and_covers_its_edges():
    repeat = 0
    for c in K.CASES:
        _, _, st = K.reference(c)
        assert st.near_edge == 0, (K.case_id(c), st.near_edge)
        assert st.pairs > 0, K.case_id(c)
        if c["kind"] == "repeat":
            assert st.repeat_groups > 0.3 * st.groups, (st.repeat_groups, st.groups)
            repeat += 1
    assert repeat and len({K.case_id(c) for c in K.CASES}) == len(K.CASES)
    counts, tokens, offsets, _, _, _, _, st = K.disjoint_case()
    assert st.near_edge == 0 and st.pairs > 50000 and (np.diff(offsets) == 0).sum() == 4 and (tokens < 0).any()
    blocks = tokens[tokens >= 0] // K.BLOCK                  # every sentence inside its own block of vocabulary ids
    assert np.array_equal(blocks, np.repeat(np.arange(K.N_SENT), np.diff(offsets))[tokens >= 0])
    from n2v_hip.sgns import _row_stride
    assert {64, 128, 256, 512} <= {_row_stride(c["dim"]) for c in K.WHOLE if c["dim"] < _row_stride(c["dim"])}
    for key, want in (("negative", {0, 1, 5, 6, 8, 15, 64}), ("window", {1, 3, 10, 17}), ("sample", {0, 1e-3, 1e-2}),
                      ("predraw", {True, False}), ("sentences_base", {0, 777, 1999})):
        assert want <= {c[key] for c in K.WHOLE}, key
    assert {0, 1, 2, 63, 64, 65, 130, 4096} <= {n for c in K.WHOLE for n in c["lens"]}
    assert any(c["seed"] >= 2**63 and c["sid_base"] == 2**40 for c in K.WHOLE) and any(c["minus1"] for c in K.WHOLE)
    assert all(c["chunk"] == 0 for c in K.WHOLE)
    shapes = {(c["chunk"], c["window"], n) for c in K.CHUNKED for n in c["lens"]}
    assert {(2, 3, 7), (1, 1, 5), (64, 10, 63), (64, 10, 64), (64, 10, 65), (64, 10, 129), (256, 5, 4096)} <= shapes
    assert any(c["first_item"] > 0 for c in K.CHUNKED)
    assert [c for c in K.CHUNKED if c["lens"] == (4096,)][0]["sample"] > 0
    # the "sparse" case: sub-sampling leaves fewer tokens than the sentence has items, yet some pairs
    c = [c for c in K.CHUNKED if c["kind"] == "sparse"][0]
    counts, tokens, offsets, _, _ = K.case_data(c)
    kw = K.ref_kwargs(c, counts)
    n_eff = len(R.effective_sentence(tokens, len(tokens), kw["sample_int"], c["seed"], c["sid_base"]))
    assert 2 <= n_eff < len(G.item_table(offsets, c["chunk"]))


# ---- (e) the C-ABI -----------------------------------------------------------------------------------------------------

def test_symbol_is_declared_bound_and_exported():
    from n2v_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "n2v_hip.h")).read()
    doc = hdr[hdr.index("skip-gram (sg=1) over the same RAGGED corpus"):hdr.index("int n2v_sgns_csr_train")]
    assert "unpinned" in doc and "csrc/n2v_sgns.hip" in doc
    assert re.search(r"#define N2V_ABI_VERSION 5\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    name = "n2v_sgns_csr_train"
    assert name in set(re.findall(r"\b(n2v_[a-z0-9_]+)\s*\(", hdr)) and name in _lib.SIGNATURES
    params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1)
    assert len(_lib.SIGNATURES[name][1]) == params.count(",") + 1 == 33
    lib = _lib.load()
    assert hasattr(lib, name) and lib.n2v_abi_version() == 5
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "n2v_sgns_csr.hip" in mk
    # one pair step: the centre step is defined once, in the shared header; both skip-gram kernels call it, and the
    # ragged one loads, reduces and adds no row of its own
    src = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
    defined = {f: len(re.findall(r"\bvoid\s+sg_centre_step\s*\(", txt)) for f, txt in src.items()}
    assert {f: n for f, n in defined.items() if n} == {"n2v_w2v_device.h": 1}, defined
    for f in ("n2v_sgns.hip", "n2v_sgns_csr.hip"):
        assert len(re.findall(r"\bsg_centre_step<", src[f])) == 1, f
    for own in ("load_row<", "add_row<", "reduce8("):
        assert own not in src["n2v_sgns_csr.hip"], own


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """Every call below returns before the first HIP call: no GPU is needed (and none is touched)."""
    from n2v_hip import _lib
    lib = _lib.load()
    one = 8     # a non-NULL "pointer" that is never dereferenced: each call fails its argument checks first

    def train(n_sent=3, n_tokens=30, max_len=64, item_off=one, chunk=16, first=0, n_items=3, n_words=50, dim=100,
              stride=128, window=5, negative=5, mode=2, total=10, batch=1, step=1, base=0, lut_bits=20, tokens=one,
              syn0=one, cum=one):
        return lib.n2v_sgns_csr_train(tokens, one, n_sent, n_tokens, max_len, item_off, chunk, first, n_items, syn0, one,
                                      n_words, dim, stride, window, negative, None, cum, one, lut_bits, 0.025, 1e-4, base,
                                      step, total, batch, 1, 0, None, mode, 1, None, None)

    for kw, msg in ((dict(n_sent=-1), "bad size"), (dict(n_tokens=-1), "bad size"), (dict(n_words=0), "bad size"),
                    (dict(n_words=2**31), "bad size"), (dict(dim=0), "bad size"), (dict(window=0), "bad size"),
                    (dict(negative=65), "bad size"), (dict(negative=-1), "bad size"),
                    (dict(max_len=0), "max_len"), (dict(max_len=4097), "max_len"),
                    (dict(chunk=-1), "chunk -1 is negative"),
                    (dict(chunk=4096), "slot"), (dict(chunk=4087, window=5), "slot"), (dict(chunk=64, window=2017), "slot"),
                    (dict(chunk=2**31 - 1, window=2**31 - 1), "slot"),
                    (dict(mode=0), "update_mode"), (dict(mode=1), "update_mode"), (dict(mode=6), "update_mode"), (dict(mode=10), "update_mode"),
                    (dict(stride=96), "row_stride"), (dict(stride=64), "row_stride"), (dict(dim=600, stride=640), "row_stride"),
                    (dict(lut_bits=0), "lut_bits"), (dict(lut_bits=25), "lut_bits"),
                    (dict(total=0), "schedule"), (dict(batch=0), "schedule"), (dict(step=0), "schedule"), (dict(base=-1), "schedule"),
                    (dict(item_off=None), "item_off missing"),
                    (dict(first=-1), "item range"), (dict(n_items=-1), "item range"), (dict(first=29, n_items=2), "item range"),
                    (dict(first=31, n_items=0), "item range"), (dict(chunk=0, item_off=None, first=1, n_items=3), "item range"),
                    (dict(chunk=0, item_off=None, first=2**62, n_items=2**62), "item range"),
                    (dict(tokens=None), "null pointer"), (dict(syn0=None), "null pointer"), (dict(cum=None), "null pointer")):
        assert train(**kw) == -1, kw
        assert msg in lib.n2v_last_error().decode(), (kw, lib.n2v_last_error())
    # the largest slot that is allowed passes the slot check (and fails the next one it is given)
    assert train(chunk=4086, window=5, mode=0) == -1 and "update_mode" in lib.n2v_last_error().decode()
    # nothing to do is no error, and needs no pointer
    assert train(n_items=0, tokens=None) == 0 and train(n_sent=0, n_items=0, n_tokens=0, tokens=None) == 0


# ---- (f) argument errors -----------------------------------------------------------------------------------------------

def test_skipgram_argument_errors():
    from n2v_hip.corpus import SentenceCorpus
    from n2v_hip.word2vec import SkipGram, Word2Vec
    with pytest.raises(NotImplementedError, match="main.learn_embeddings"):
        Word2Vec([["a", "b"]], sg=1)
    assert "SkipGram" in Word2Vec.__doc__
    for kw in (dict(size=0), dict(size=513), dict(iter=0), dict(window=0), dict(negative=65), dict(negative=-1),
               dict(chunk=-1), dict(chunk="big"), dict(chunk=1.5), dict(chunk=True), dict(chunk=4087), dict(chunk=64, window=2017)):
        with pytest.raises(ValueError):
            SkipGram([["a", "b"]], **kw)
    with pytest.raises(ValueError, match="vocabulary is empty"):
        SkipGram(SentenceCorpus.from_sentences([["a", "b"]], min_count=2, device="cpu"))
    with pytest.raises(ValueError):
        SentenceCorpus.from_sentences([["a", "b"]], min_count=-1, device="cpu")


def test_models_share_their_tables_code():
    from n2v_hip import cbow, skipgram
    assert issubclass(skipgram.SkipGramModel, cbow.RaggedModel) and issubclass(cbow.CbowModel, cbow.RaggedModel)
    for name in ("build_vocab", "reset_weights", "vectors"):
        assert getattr(skipgram.SkipGramModel, name) is getattr(cbow.CbowModel, name), name
    assert skipgram.SkipGramModel.train_pass is not cbow.CbowModel.train_pass
    with pytest.raises(ValueError):
        skipgram.SkipGramModel(0)
    with pytest.raises(ValueError):
        skipgram.SkipGramModel(5, window=0)


def test_extract_playlist_has_the_sg_flag_and_defaults_to_cbow(monkeypatch):
    import extract_playlist as E
    a = E.parse_args(["-input", "x"])
    assert a.sg == 0 and a.chunk == "auto"
    a = E.parse_args(["-input", "x", "-sg", "1", "-chunk", "64"])
    assert a.sg == 1 and a.chunk == 64 and E.parse_args(["-input", "x", "-chunk", "0"]).chunk == 0
    for bad in (["-sg", "2"], ["-chunk", "-1"], ["-chunk", "big"]):
        with pytest.raises(SystemExit):
            E.parse_args(["-input", "x"] + bad)
    seen = []
    monkeypatch.setattr(E._word2vec, "SkipGram", lambda s, **kw: seen.append(("sg", kw)))
    monkeypatch.setattr(E._word2vec, "Word2Vec", lambda s, **kw: seen.append(("cbow", kw)))
    E.train_song2vec([["a"]], 3, sg=1, size=8, chunk=64)
    E.train_song2vec([["a"]], 3, size=8, chunk=64)
    E.train_song2vec([["a"]], 4)
    assert seen == [("sg", dict(min_count=3, size=8, chunk=64)), ("cbow", dict(min_count=3, size=8)), ("cbow", dict(min_count=4))]
    with pytest.raises(ValueError):
        E.train_song2vec([["a"]], 3, sg=2)


# ---- (g) the kernel compiles for gfx950 without scratch ------------------------------------------------------------------

def test_kernel_cross_compiles_for_gfx950_without_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the kernel cannot be compiled")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
                          os.path.join(CSRC, "n2v_sgns_csr.hip"), "-o", os.path.join(str(tmp_path), "k.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*sgns_csr_kernel\S*)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert len(names) == 8 == len(set(names)) and len(scratch) == 8, names
    assert scratch == [0] * 8, dict(zip(names, scratch))
