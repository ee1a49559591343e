'''
Drop-in for the reference's ``src/extract_playlist.py`` on MI355X: ``extract_playlist(rows)`` cuts the 30Music
event log into playlists and ``train_song2vec(sentences, min_ct)`` trains song2vec — gensim's
``Word2Vec(sentences, min_count=min_ct)`` (CBOW) — with the HIP kernel of n2v_hip/cbow.py, or with ``-sg 1`` skip-gram
over the same playlists (n2v_hip/skipgram.py).

    python extract_playlist.py -input events.csv -min-count 5 -output emb/song2vec.emb [-size 100 -window 5 -iter 5 -seed 1]
                               [-sg {0,1}] [-chunk auto|N]

The event file has ``import_30``'s columns (src/utils.py:22-30): eid,timestamp,playtime,uid,id — no header, quotes
stripped.
'''
import argparse
import os

from n2v_hip import playlist as _playlist
from n2v_hip import word2vec as _word2vec

COLUMNS = ("eid", "timestamp", "playtime", "uid", "id")


def import_30(path):
    """-> dict of column lists (strings), src/utils.py:22-30."""
    with open(path, "r") as f:
        data = [x.replace('"', "").strip("\n").split(",") for x in f.readlines()]
    data = [r for r in data if r != [""]]
    for r in data:
        if len(r) != len(COLUMNS):
            raise ValueError("%s: expected %d columns (%s), got %r" % (path, len(COLUMNS), ",".join(COLUMNS), r))
    return {c: [r[i] for r in data] for i, c in enumerate(COLUMNS)}


def extract_playlist(rows, device=None):
    """rows: dict (or DataFrame) with uid, timestamp, playtime and the track id as `tid` or `id`
    (src/extract_playlist.py:4-28) -> list of playlists, each a list of track ids."""
    tid = rows["tid"] if "tid" in rows else rows["id"]
    return _playlist.extract_playlists(list(rows["uid"]), [int(x) for x in rows["timestamp"]],
                                       [int(x) for x in rows["playtime"]], list(tid), device=device)


def train_song2vec(sentences, min_ct, sg=0, **kw):
    """src/extract_playlist.py:31-34; sg=1: skip-gram over the same playlists (`chunk` as n2v_hip.word2vec.SkipGram)."""
    if sg not in (0, 1):
        raise ValueError("sg must be 0 (CBOW) or 1 (skip-gram)")
    if sg == 1:
        return _word2vec.SkipGram(sentences, min_count=min_ct, **kw)
    kw.pop("chunk", None)
    return _word2vec.Word2Vec(sentences, min_count=min_ct, **kw)


def _chunk_arg(text):
    if text == "auto":
        return text
    value = int(text)
    if value < 0:
        raise argparse.ArgumentTypeError("-chunk must be 'auto' or an int >= 0")
    return value


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="song2vec on MI355X")
    ap.add_argument("-input", required=True, help="30Music event file (eid,timestamp,playtime,uid,id)")
    ap.add_argument("-min-count", dest="min_count", type=int, default=5)
    ap.add_argument("-output", default="emb/song2vec.emb", help="word2vec text format")
    ap.add_argument("-size", type=int, default=100)
    ap.add_argument("-window", type=int, default=5)
    ap.add_argument("-iter", type=int, default=5)
    ap.add_argument("-seed", type=int, default=1)
    ap.add_argument("-sg", type=int, choices=(0, 1), default=0, help="0: CBOW (the reference's song2vec), 1: skip-gram")
    ap.add_argument("-chunk", type=_chunk_arg, default="auto",
                    help="skip-gram only: centres per work item (auto, or an int; 0 = whole sentences)")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    sentences = extract_playlist(import_30(a.input))
    song2vec = train_song2vec(sentences, a.min_count, sg=a.sg, size=a.size, window=a.window, iter=a.iter, seed=a.seed,
                              chunk=a.chunk)
    d = os.path.dirname(a.output)
    if d:
        os.makedirs(d, exist_ok=True)
    song2vec.save_word2vec_format(a.output)
    print("song2vec: %d playlists, %d tracks, %d %s trained -> %s"
          % (len(sentences), len(song2vec.wv.vocab), song2vec.pairs_trained, "pairs" if a.sg else "centres", a.output))
    return song2vec


if __name__ == "__main__":
    main()
