"""Drop-in for the working part of the reference's src/main_rec.py: EccenKNN rating prediction on the device.

    python main_rec.py -input ratings.csv [-k 40] [-mink 1] [-sim cosine|msd] [-item-based] [-weights FILE]
                       [-test-ratio 0.2] [-seed 0] [-cv N]

-input    csv `user,item,rating[,timestamp]`, an optional header line is skipped
-weights  `id,weight` lines for the y side (items, or users with -item-based); absent = all ones, which is plain k-NN.
          The reference derives them with pandas (src/utils.py:95-153); here they are an input.
The split is seeded: a permutation of the ratings by numpy's RandomState(seed), the first round(n * ratio) of it are
the test set and the rest, in file order, the training set.  -cv N runs N folds of the same permutation instead.
Prints `RMSE: <repr>` per split (and their mean for -cv).
"""
import argparse
import sys

import numpy as np


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="EccenKNN rating prediction (HIP, gfx950)")
    p.add_argument("-input", required=True)
    p.add_argument("-k", type=int, default=40)
    p.add_argument("-mink", type=int, default=1)
    p.add_argument("-sim", default="cosine")
    p.add_argument("-item-based", dest="item_based", action="store_true")
    p.add_argument("-min-support", dest="min_support", type=int, default=1)
    p.add_argument("-weights", default=None)
    p.add_argument("-test-ratio", dest="test_ratio", type=float, default=0.2)
    p.add_argument("-seed", type=int, default=0)
    p.add_argument("-cv", type=int, default=0)
    p.add_argument("-device", default="cuda:0")
    a = p.parse_args(argv)
    if not 0.0 < a.test_ratio < 1.0:
        p.error("-test-ratio must be inside (0, 1)")
    if a.cv == 1 or a.cv < 0:
        p.error("-cv needs at least 2 folds")
    return a


def read_ratings(path):
    """(users, items, ratings) of a csv; ids stay strings, a first line whose rating is no number is a header."""
    users, items, ratings = [], [], []
    with open(path) as f:
        for n, line in enumerate(f):
            parts = line.strip().split(",")
            if len(parts) < 3:
                if line.strip():
                    raise ValueError("%s:%d: expected user,item,rating[,timestamp]" % (path, n + 1))
                continue
            try:
                r = float(parts[2])
            except ValueError:
                if n == 0:
                    continue
                raise
            users.append(parts[0]); items.append(parts[1]); ratings.append(r)
    return users, items, np.array(ratings, dtype=np.float64)


def read_weights(path):
    out = {}
    with open(path) as f:
        for n, line in enumerate(f):
            parts = line.strip().split(",")
            if len(parts) < 2:
                continue
            try:
                out[parts[0]] = float(parts[1])
            except ValueError:
                if n:
                    raise
    return out


def split(n, ratio, seed):
    """(train index ascending, test index in permutation order)."""
    perm = np.random.RandomState(seed).permutation(n)
    n_test = int(round(n * ratio))
    return np.sort(perm[n_test:]), perm[:n_test]


def folds(n, n_folds, seed):
    perm = np.random.RandomState(seed).permutation(n)
    for part in np.array_split(perm, n_folds):
        yield np.sort(np.setdiff1d(perm, part)), part


def run_split(args, users, items, ratings, weights, train, test):
    from n2v_hip import eccknn
    ts = eccknn.Trainset.from_ratings([users[i] for i in train], [items[i] for i in train], ratings[train],
                                      rating_scale=(float(ratings.min()), float(ratings.max())))
    algo = eccknn.EccenKNN(k=args.k, min_k=args.mink, device=args.device,
                           sim_options={"name": args.sim, "user_based": not args.item_based, "min_support": args.min_support})
    if weights is None:
        w = np.ones(ts.n_users if args.item_based else ts.n_items)
    else:
        w = weights
    algo.fit(ts, w)
    return algo.rmse([(users[i], items[i], ratings[i]) for i in test])


def main(argv=None):
    args = parse_args(argv)
    users, items, ratings = read_ratings(args.input)
    weights = read_weights(args.weights) if args.weights else None
    if args.cv:
        errs = []
        for train, test in folds(len(ratings), args.cv, args.seed):
            errs.append(run_split(args, users, items, ratings, weights, train, test))
            print("RMSE: %r" % errs[-1])
        print("mean RMSE: %r" % float(np.mean(errs)))
        return errs
    train, test = split(len(ratings), args.test_ratio, args.seed)
    err = run_split(args, users, items, ratings, weights, train, test)
    print("RMSE: %r" % err)
    return err


if __name__ == "__main__":
    main(sys.argv[1:])
