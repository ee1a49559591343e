"""Drop-in for the working part of the reference's src/main_ecc.py: the eccentricity split of a ratings file.

    python main_ecc.py -input ratings.csv [-split-n 10] [-out DIR] [-prefix P] [-window-col timestamp|timewindow]
                       [-save-bins FILE] [-embed DIR --num-walks 3 --walk-length 40 --dimensions 128 --window-size 10
                        --iter 1 --p 1 --q 1 --rng numpy|philox --seed 1] [-device cuda:0]
                       [-similar-emb EMB -similar-ratio R [-similar-target UID] [-similar-name cosine_onetenth]]

The reference (src/main_ecc.py:32-38, :65-74, :112-117) reads ./data/ratings.csv, computes every user's eccentricity
ue, marks the users with `split_n` equal bins by ue and writes ./graph/ml/ue.edgelist and ue_1.edgelist .. ue_n.edgelist,
which split_embedding.sh then embeds one by one (src/main.py --weighted --num-walks 3 --walk-length 40).  Its other
branches do not run (a syntax error at :127-130) and are not restated.  Here ue (n2v_hip.eccstats), the bins and the
n + 1 graphs (n2v_hip.eccsplit) are computed on the device.

-input       csv `user,item,rating,timestamp`, an optional header line is skipped; ids must be integers
-split-n     number of bins (the reference's -split_n, default 10)
-out         write the reference's files there, byte for byte (<prefix>ue.edgelist, <prefix>ue_<k>.edgelist)
-window-col  the 4th column is a unix timestamp, cut into UTC months (default), or the time window itself
-save-bins   write `uid,ue,bin` lines
-embed       embed every non-empty graph as split_embedding.sh does, straight from the in-memory graph (no file is
             read back), and write DIR/<prefix>ue.emb, DIR/<prefix>ue_<k>.emb in word2vec text format
-similar-emb the similar-users subgraph (src/main_ecc.py:102-104, src/utils.py:428-456): the int(R * n_users) users of the
             word2vec text file EMB nearest to one user by cosine (n2v_hip.neighbors.find_similar_users; -similar-target,
             default a choice seeded by --seed) and, with -out, <prefix><name>.edgelist of their rows
Prints one line per graph: its name, nodes and adjacency entries.
"""
import argparse
import os


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="eccentricity split of a ratings file (HIP, gfx950)")
    p.add_argument("-input", required=True)
    p.add_argument("-split-n", "-split_n", dest="split_n", type=int, default=10)
    p.add_argument("-out", default=None)
    p.add_argument("-prefix", default="")
    p.add_argument("-window-col", dest="window_col", default="timestamp", choices=["timestamp", "timewindow"])
    p.add_argument("-save-bins", dest="save_bins", default=None)
    p.add_argument("-embed", default=None)
    p.add_argument("-device", default="cuda:0")
    p.add_argument("-similar-emb", dest="similar_emb", default=None)
    p.add_argument("-similar-ratio", dest="similar_ratio", type=float, default=None)
    p.add_argument("-similar-target", dest="similar_target", default=None)
    p.add_argument("-similar-name", dest="similar_name", default="cosine_onetenth")
    # split_embedding.sh's command line; everything else as src/main.py's defaults
    p.add_argument("--num-walks", dest="num_walks", type=int, default=3)
    p.add_argument("--walk-length", dest="walk_length", type=int, default=40)
    p.add_argument("--dimensions", type=int, default=128)
    p.add_argument("--window-size", dest="window_size", type=int, default=10)
    p.add_argument("--iter", type=int, default=1)
    p.add_argument("--p", type=float, default=1)
    p.add_argument("--q", type=float, default=1)
    p.add_argument("--rng", default="numpy", choices=["numpy", "philox"])
    p.add_argument("--seed", type=int, default=1)
    a = p.parse_args(argv)
    if a.split_n < 1:
        p.error("-split-n must be at least 1")
    if not (a.out or a.embed or a.save_bins):
        p.error("nothing to do: give -out, -embed or -save-bins")
    if (a.similar_emb is None) != (a.similar_ratio is None):
        p.error("-similar-emb and -similar-ratio go together")
    if a.similar_emb is not None and not a.out:
        p.error("-similar-emb writes its edge list under -out")
    for name in ("num_walks", "walk_length", "dimensions", "window_size", "iter"):
        if getattr(a, name) < 1:
            p.error("--%s must be at least 1" % name.replace("_", "-"))
    return a


def write_bins(path, split):
    with open(path, "w") as f:
        for uid, ue in zip(split.users, split.ue.tolist()):
            f.write("%s,%r,%d\n" % (uid, ue, split.bins[uid]))


def embed(split, a):
    """split_embedding.sh over the in-memory graphs: {file stem: path of the .emb written}."""
    import main as n2v_main
    import node2vec
    os.makedirs(a.embed, exist_ok=True)
    n2v_main.args = argparse.Namespace(dimensions=a.dimensions, window_size=a.window_size, iter=a.iter, seed=a.seed)
    written = {}
    for name, g in zip(split.file_names(a.prefix), split.graphs):
        if g.n_nodes == 0:
            continue
        G = node2vec.Graph.from_csr(g, a.p, a.q, device=a.device, rng=a.rng, seed=a.seed)
        G.preprocess_transition_probs()
        walks = G.simulate_walks(a.num_walks, a.walk_length)
        stem = name[:-len(".edgelist")]
        written[stem] = os.path.join(a.embed, stem + ".emb")
        n2v_main.save_embeddings(n2v_main.learn_embeddings(walks), written[stem])
    return written


def similar_users_graph(split, a):
    """<out>/<prefix><name>.edgelist: the rows of the users find_similar_users names, in file order."""
    from n2v_hip import neighbors
    similar = neighbors.find_similar_users(a.similar_emb, a.similar_ratio, target=a.similar_target, seed=a.seed,
                                           device=a.device)
    rows = split.rows_of_users(similar)
    g = split.graph_of_rows(rows, device=a.device)
    name = a.prefix + a.similar_name + ".edgelist"
    print("%s: %d nodes, %d entries" % (name, g.n_nodes, g.nnz))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, name), "w") as f:
        f.write(split.edgelist_text(rows=rows))
    return similar


def main(a):
    import main_rec
    from n2v_hip import eccsplit
    users, items, ratings = main_rec.read_ratings(a.input)
    windows = main_rec.read_windows(a.input, a.window_col)
    split = eccsplit.split(users, items, ratings, windows, n=a.split_n, device=a.device)
    for name, g in zip(split.file_names(a.prefix), split.graphs):
        print("%s: %d nodes, %d entries" % (name, g.n_nodes, g.nnz))
    if a.out:
        split.write(a.out, a.prefix)
    if a.save_bins:
        write_bins(a.save_bins, split)
    if a.embed:
        embed(split, a)
    if a.similar_emb:
        similar_users_graph(split, a)
    return split


if __name__ == "__main__":
    main(parse_args())
