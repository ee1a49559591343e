"""Drop-in for the working part of the reference's src/main_rec.py: EccenKNN rating prediction on the device, and the
plain k-NN (surprise's KNNBasic) it is compared against.

    python main_rec.py -input ratings.csv [-algo eccen|knn|knnmeans|knnzscore|knnbaseline] [-k 40] [-mink 1] [-sim cosine|msd|pearson|pearson_baseline]
                       [-shrinkage 100] [-item-based] [-weights FILE]
                       [-mode ir|ie|ire|ier] [-window-col timestamp|timewindow] [-save-weights FILE]
                       [-test-ratio 0.2] [-seed 0] [-cv N] [-form auto|dense|sparse]
                       [-sweep-k 5,10,20,40,80 [-sweep-mink 1,5]]
    python main_rec.py -input ratings.csv -algo mf [-factors 100] [-epochs 20] [-lr 0.005] [-reg 0.02] [-strata N|auto]
                       [-unbiased] [-test-ratio 0.2] [-seed 0] [-cv N]
    python main_rec.py -input ratings.csv -algo nmf [-factors 15] [-epochs 50] [-reg 0.06] [-test-ratio 0.2] [-seed 0] [-cv N]
    python main_rec.py -input ratings.csv -algo slopeone [-form auto|dense|sparse] [-test-ratio 0.2] [-seed 0] [-cv N]
    python main_rec.py -input ratings.csv -algo coclustering [-clusters-u 3] [-clusters-i 3] [-epochs 20] [-test-ratio 0.2]
                       [-seed 0] [-cv N]
    every form:        [-topn N [-threshold T] [-save-recs FILE]] [-mae]

-input    csv `user,item,rating[,timestamp]`, an optional header line is skipped
-algo     eccen (the default) or knn: KNNBasic, which also takes -sim pearson and pearson_baseline (surprise's functions,
          restated; parity with surprise is unpinned) and -shrinkage for the latter.  With -algo knn, -weights / -mode
          weight the baseline's co-ratings, as the reference meant to (src/main_rec.py:197); absent, there are no weights.
          mf: matrix factorisation, the model and SGD update of surprise's SVD (restated; parity with surprise is
          unpinned) trained on the device under a deterministic stratified order of the ratings (n2v_hip.svd): -factors,
          -epochs, -lr and -reg are surprise's n_factors, n_epochs, lr_all and reg_all, -strata the number of strata (auto:
          chosen from the size of the training set; 1: surprise's own order), -unbiased drops the biases, and -seed also
          seeds the factors.  It takes none of -sim, -k, -mink, -weights, -mode, -item-based and -form.
          knnmeans, knnzscore, knnbaseline: surprise's KNNWithMeans, KNNWithZScore and KNNBaseline (restated; parity with
          surprise is unpinned), the centred k-NN predictors: the neighbours of knn, each neighbour's rating taken relative
          to its row mean, to its row mean in units of its row sigma, or to the ALS baseline of the pair, and too few
          neighbours leave the base estimate instead of the training mean.  They take every flag -algo knn takes, -weights /
          -mode included (the eccentricity-weighted, centred k-NN), and none of the mf flags.
          nmf: surprise's NMF (restated; parity with surprise is unpinned), the non-negative factor model with the
          multiplicative update, trained on the device in surprise's own order of the ratings (n2v_hip.nmf): -factors,
          -epochs and -reg are surprise's n_factors, n_epochs and reg_pu = reg_qi, and -seed also seeds the factors.  It
          has no biases, no learning rate and no schedule: it takes none of -lr, -strata, -unbiased and the k-NN flags.
          slopeone: surprise's SlopeOne (restated; parity with surprise is unpinned), the parameter-free baseline: the mean
          difference of every pair of items over the users who rated both, fitted on the device by the co-rated pair pass of
          the similarities (n2v_hip.slopeone), and a prediction is the user's mean plus the mean difference to the items
          they rated.  It has no hyper-parameter and no random state: beside the split, -topn and -device flags it takes
          -form alone, and none of -k, -mink, -sim, -shrinkage, -weights, -mode, -item-based and the factor flags.
          coclustering: surprise's CoClustering (restated; parity with surprise is unpinned): users and items are each
          put into clusters, and a prediction is the co-cluster's average plus what the user's and the item's mean differ
          from their clusters' averages; trained on the device in surprise's own order of the ratings, every user and then
          every item reassigned in parallel (n2v_hip.coclustering).  -clusters-u, -clusters-i and -epochs are surprise's
          n_cltr_u, n_cltr_i (1 .. 64 each) and n_epochs, and -seed also seeds the first assignment.  It takes none of
          the k-NN flags, -form, -shrinkage, -factors, -lr, -reg, -strata and -unbiased.
          svd itself is not built: surprise's order of the ratings is sequential, and -algo mf follows it only with -strata 1.
-weights  `id,weight` lines for the y side (items, or users with -item-based); absent = all ones, which is plain k-NN.
-mode     derive the item weights on the device instead (n2v_hip.eccstats; the reference's src/utils.py:95-153): item
          rarity, item eccentricity, their product or their quotient, from the WHOLE input file before the split, as the
          reference's fit does.  Needs the 4th column: a unix timestamp, cut into UTC months (-window-col timestamp, the
          default; the reference cuts in the machine's local zone) or the time window itself (-window-col timewindow).
          Conflicts with -weights and with -item-based (the reference keys the weights by item there while y is a user).
-save-weights  write the `id,weight` lines that were used, in the form -weights reads.
-form     the similarity kernel: dense (n_x * n_y at most 2^31), sparse (rating lists, no such limit), auto = dense inside it.
The split is seeded: a permutation of the ratings by numpy's RandomState(seed), the first round(n * ratio) of it are
the test set and the rest, in file order, the training set.  -cv N runs N folds of the same permutation instead.
Prints `RMSE: <repr>` per split (and their mean for -cv).
-topn     with every -algo: after each split's RMSE line, rank for every test user the N training items they have not
          rated by predicted rating (equal predictions by first appearance in the training data; fused on the device,
          the users x items predictions are never stored) and print `F1 / MAP / MRR / NDCG @N: ...` against the split's
          test set (the metrics of BiNE's top_N).  1 <= N <= 256.  main() then returns (rmse, (f1, map, mrr, ndcg)) per split.
-threshold  only test items rated at least T are a user's ground truth (absent: all of them); users left without any
          are not counted.
-save-recs  write `user,item,score` lines, every training user's list best first; under -cv one file per fold, FILE.0,
          FILE.1, ...
-mae      with every -algo: one more line `MAE: <repr>` after each split's `RMSE:` line (and `mean MAE:` for -cv), the mean
          absolute error of the same predictions, the second measure of surprise's cross_validate.  What main() returns
          does not change.
-sweep-k  with -algo eccen and the four k-NN algos: the reference's experiment, every neighbourhood size of the list
          (1 to 16 values, strictly ascending, each at most 256) against every -sweep-mink (the same rules; absent: the
          run's -mink alone) on each split.  A split is fitted once and all cells come from one neighbour selection at the
          largest k (n2v_hip.eccknn.estimate_sweep), each with the numbers a run with that -k and -mink prints.  Prints
          `k K mink M RMSE: <repr> MAE: <repr>` per cell in grid order; with -cv, after the folds, `k K mink M mean RMSE:
          <repr> mean MAE: <repr>` per cell; then `best: k K mink M mean RMSE <repr>`, the smallest mean RMSE, ties to
          the smaller k and then the smaller min_k.  main() then returns {(k, min_k): {"rmse", "mae"}} per split.  -k
          plays no part.  It does not go with -topn.
"""
import argparse
import sys

import numpy as np


KNN_ALGOS = ("knn", "knnmeans", "knnzscore", "knnbaseline")     # surprise's KNNBasic and its three centred siblings


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="EccenKNN / KNNBasic rating prediction (HIP, gfx950)")
    p.add_argument("-input", required=True)
    p.add_argument("-algo", default="eccen")
    p.add_argument("-shrinkage", type=float, default=None)
    p.add_argument("-k", type=int, default=None)
    p.add_argument("-mink", type=int, default=None)
    p.add_argument("-sim", default=None)
    p.add_argument("-item-based", dest="item_based", action="store_true")
    p.add_argument("-min-support", dest="min_support", type=int, default=1)
    p.add_argument("-weights", default=None)
    p.add_argument("-mode", default=None, choices=["ir", "ie", "ire", "ier"])
    p.add_argument("-window-col", dest="window_col", default="timestamp", choices=["timestamp", "timewindow"])
    p.add_argument("-save-weights", dest="save_weights", default=None)
    p.add_argument("-test-ratio", dest="test_ratio", type=float, default=0.2)
    p.add_argument("-seed", type=int, default=0)
    p.add_argument("-cv", type=int, default=0)
    p.add_argument("-form", default=None, choices=["auto", "dense", "sparse"])
    p.add_argument("-factors", type=int, default=None)
    p.add_argument("-epochs", type=int, default=None)
    p.add_argument("-lr", type=float, default=None)
    p.add_argument("-reg", type=float, default=None)
    p.add_argument("-strata", default=None)
    p.add_argument("-unbiased", action="store_true")
    p.add_argument("-clusters-u", dest="clusters_u", type=int, default=None)
    p.add_argument("-clusters-i", dest="clusters_i", type=int, default=None)
    p.add_argument("-device", default="cuda:0")
    p.add_argument("-topn", type=int, default=None)
    p.add_argument("-threshold", type=float, default=None)
    p.add_argument("-save-recs", dest="save_recs", default=None)
    p.add_argument("-sweep-k", dest="sweep_k", default=None)
    p.add_argument("-sweep-mink", dest="sweep_mink", default=None)
    p.add_argument("-mae", action="store_true")
    a = p.parse_args(argv)
    if a.topn is None:
        for flag, v in (("-threshold", a.threshold), ("-save-recs", a.save_recs)):
            if v is not None:
                p.error("%s needs -topn" % flag)
    else:
        from n2v_hip import eccknn
        try:
            eccknn.topn_options(a.topn, None)
            eccknn.threshold_option(a.threshold)
        except ValueError as e:
            p.error("-topn / -threshold: %s" % e)
    if a.algo == "svd":
        p.error("-algo svd is not built: surprise's SVD applies the ratings in one sequential order.  -algo mf is the same "
                "model and update under a deterministic stratified order (equal to surprise's only with -strata 1)")
    if a.algo not in ("eccen", "mf", "nmf", "slopeone", "coclustering") + KNN_ALGOS:
        p.error("-algo %s: eccen, %s, mf, nmf, slopeone or coclustering" % (a.algo, ", ".join(KNN_ALGOS)))
    knn_flags = (("-sim", a.sim), ("-k", a.k), ("-mink", a.mink), ("-weights", a.weights), ("-mode", a.mode),
                 ("-item-based", a.item_based or None), ("-form", a.form))
    mf_flags = (("-factors", a.factors), ("-epochs", a.epochs), ("-lr", a.lr), ("-reg", a.reg), ("-strata", a.strata),
                ("-unbiased", a.unbiased or None))
    sgd_flags = tuple(f for f in mf_flags if f[0] in ("-lr", "-strata", "-unbiased"))     # what mf has and nmf has not
    slope_flags = tuple(f for f in knn_flags if f[0] != "-form") + (("-shrinkage", a.shrinkage),) + mf_flags   # all but -form
    cocl_flags = tuple(f for f in knn_flags + (("-shrinkage", a.shrinkage),) + mf_flags if f[0] != "-epochs")   # all but -epochs
    cluster_flags = (("-clusters-u", a.clusters_u), ("-clusters-i", a.clusters_i))
    refused = {"mf": knn_flags, "nmf": knn_flags + sgd_flags, "slopeone": slope_flags, "coclustering": cocl_flags}
    for flag, v in refused.get(a.algo, mf_flags) + (() if a.algo == "coclustering" else cluster_flags):
        if v is not None:
            p.error("%s does not go with -algo %s" % (flag, a.algo))
    if a.algo == "coclustering":
        from n2v_hip import coclustering
        a.clusters_u, a.clusters_i = (3 if v is None else v for v in (a.clusters_u, a.clusters_i))
        try:
            coclustering.CoClustering(n_cltr_u=a.clusters_u, n_cltr_i=a.clusters_i, n_epochs=20 if a.epochs is None else a.epochs)
        except ValueError as e:
            p.error(str(e))
    factor_defaults = (("factors", 15), ("epochs", 50), ("reg", 0.06)) if a.algo == "nmf" else ()
    for name, v in factor_defaults + (("shrinkage", 100), ("k", 40), ("mink", 1), ("sim", "cosine"), ("form", "auto"),
                                      ("factors", 100), ("epochs", 20), ("lr", 0.005), ("reg", 0.02), ("strata", "auto")):
        if getattr(a, name) is None:
            setattr(a, name, v)
    if a.strata != "auto":
        try:
            a.strata = int(a.strata)
        except ValueError:
            p.error("-strata %s: a number or auto" % a.strata)
    if a.algo == "mf":
        from n2v_hip import svd
        try:
            svd.SVD(n_factors=a.factors, n_epochs=a.epochs, lr_all=a.lr, reg_all=a.reg, n_strata=a.strata)
        except ValueError as e:
            p.error(str(e))
    if a.algo == "nmf":
        from n2v_hip import nmf
        try:
            nmf.NMF(n_factors=a.factors, n_epochs=a.epochs, reg_pu=a.reg, reg_qi=a.reg)
        except ValueError as e:
            p.error(str(e))
    if a.sweep_k is None:
        if a.sweep_mink is not None:
            p.error("-sweep-mink needs -sweep-k")
    else:
        if a.algo != "eccen" and a.algo not in KNN_ALGOS:
            p.error("-sweep-k does not go with -algo %s" % a.algo)
        if a.topn is not None:
            p.error("-sweep-k does not go with -topn")
        from n2v_hip import eccknn
        try:
            grid = [[int(v) for v in text.split(",")] for text in (a.sweep_k, a.sweep_mink or str(a.mink))]
            a.sweep_k, a.sweep_mink = eccknn.sweep_options(*grid)
        except ValueError as e:
            p.error("-sweep-k / -sweep-mink: %s" % e)
    if a.sim in ("pearson", "pearson_baseline") and a.algo not in KNN_ALGOS:
        p.error("-sim %s is surprise's own similarity: it needs -algo knn (or knnmeans, knnzscore, knnbaseline)" % a.sim)
    if not 0.0 < a.test_ratio < 1.0:
        p.error("-test-ratio must be inside (0, 1)")
    if a.cv == 1 or a.cv < 0:
        p.error("-cv needs at least 2 folds")
    if a.mode and a.weights:
        p.error("-mode computes the weights, -weights reads them: give one of the two")
    if a.mode and a.item_based:
        p.error("-mode weights items, and with -item-based the weighted side is the users")
    if a.save_weights and not (a.mode or a.weights):
        p.error("-save-weights: there are no weights to save without -mode or -weights")
    if a.mode:
        try:
            a.windows = read_windows(a.input, a.window_col)
        except ValueError as e:
            p.error(str(e))
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


def read_windows(path, window_col):
    """The time window of every row that read_ratings keeps: the 4th column itself, or its UTC month."""
    col = []
    with open(path) as f:
        for n, line in enumerate(f):
            parts = line.strip().split(",")
            if len(parts) < 3:
                continue
            try:
                float(parts[2])
            except ValueError:
                if n == 0:
                    continue
                raise
            if len(parts) < 4 or not parts[3].strip():
                raise ValueError("%s:%d: -mode needs the 4th column (%s) and this line has none" % (path, n + 1, window_col))
            try:
                col.append(int(parts[3]))
            except ValueError:
                col.append(int(float(parts[3])))
    col = np.array(col, dtype=np.int64)
    if window_col == "timewindow":
        return col
    from n2v_hip import eccstats
    return eccstats.timewindow_utc(col)


def write_weights(path, weights):
    with open(path, "w") as f:
        for k, v in weights.items():
            f.write("%s,%r\n" % (k, v))


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


def fit_split(args, users, items, ratings, weights, train):
    """The fitted algorithm of one split."""
    from n2v_hip import eccknn
    ts = eccknn.Trainset.from_ratings([users[i] for i in train], [items[i] for i in train], ratings[train],
                                      rating_scale=(float(ratings.min()), float(ratings.max())))
    if args.algo == "mf":
        from n2v_hip import svd
        algo = svd.SVD(n_factors=args.factors, n_epochs=args.epochs, biased=not args.unbiased, lr_all=args.lr,
                       reg_all=args.reg, random_state=args.seed, n_strata=args.strata, device=args.device)
        return algo.fit(ts)
    if args.algo == "nmf":
        from n2v_hip import nmf
        algo = nmf.NMF(n_factors=args.factors, n_epochs=args.epochs, reg_pu=args.reg, reg_qi=args.reg, random_state=args.seed,
                       device=args.device)
        return algo.fit(ts)
    if args.algo == "slopeone":
        from n2v_hip import slopeone
        return slopeone.SlopeOne(sim_options={"form": args.form}, device=args.device).fit(ts)
    if args.algo == "coclustering":
        from n2v_hip import coclustering
        algo = coclustering.CoClustering(n_cltr_u=args.clusters_u, n_cltr_i=args.clusters_i, n_epochs=args.epochs,
                                         random_state=args.seed, device=args.device)
        return algo.fit(ts)
    sim_options = {"name": args.sim, "user_based": not args.item_based, "min_support": args.min_support, "form": args.form}
    if args.algo in KNN_ALGOS:
        sim_options["shrinkage"] = args.shrinkage
        cls = {"knn": eccknn.KNNBasic, "knnmeans": eccknn.KNNWithMeans, "knnzscore": eccknn.KNNWithZScore,
               "knnbaseline": eccknn.KNNBaseline}[args.algo]
        algo = cls(k=args.k, min_k=args.mink, device=args.device, sim_options=sim_options)
        return algo.fit(ts, weights)
    algo = eccknn.EccenKNN(k=args.k, min_k=args.mink, device=args.device, sim_options=sim_options)
    if weights is None:
        w = np.ones(ts.n_users if args.item_based else ts.n_items)
    else:
        w = weights
    return algo.fit(ts, w)


def write_recs(path, recs):
    with open(path, "w") as f:
        for user, lst in recs.items():
            for item, score in lst:
                f.write("%s,%s,%r\n" % (user, item, score))


def run_split(args, users, items, ratings, weights, train, test, recs_path=None):
    """(result, mae) of one split.  result: the rmse; with -topn, (rmse, (f1, map, mrr, ndcg)), and the lists written to
    recs_path when it is given; with -sweep-k, {(k, min_k): {"rmse", "mae"}} over the grid.  mae: None without -mae."""
    algo = fit_split(args, users, items, ratings, weights, train)
    testset = [(users[i], items[i], ratings[i]) for i in test]
    if args.sweep_k is not None:
        return algo.accuracy_sweep(testset, args.sweep_k, args.sweep_mink), None
    err = algo.rmse(testset)
    mae = algo.mae(testset) if args.mae else None
    if args.topn is None:
        return err, mae
    metrics = algo.ranking_metrics(testset, args.topn, args.threshold)[:4]
    if recs_path:
        write_recs(recs_path, algo.recommend(args.topn))
    return (err, metrics), mae


def report(args, result, mae=None):
    """Prints one split's lines."""
    if args.sweep_k is not None:
        for (k, min_k), cell in result.items():
            print("k %d mink %d RMSE: %r MAE: %r" % (k, min_k, cell["rmse"], cell["mae"]))
        return
    print("RMSE: %r" % (result if args.topn is None else result[0]))
    if mae is not None:
        print("MAE: %r" % mae)
    if args.topn is not None:
        print("F1 / MAP / MRR / NDCG @%d: %r / %r / %r / %r" % ((args.topn,) + tuple(result[1])))


def report_sweep(args, results):
    """After the splits of a sweep: the per-cell means when there are folds, then the best cell by mean RMSE, ties to the
    smaller k and then the smaller min_k (the grid's order)."""
    cells = [(k, min_k) for k in args.sweep_k for min_k in args.sweep_mink]
    mean = {c: tuple(float(np.mean([r[c][m] for r in results])) for m in ("rmse", "mae")) for c in cells}
    if args.cv:
        for c in cells:
            print("k %d mink %d mean RMSE: %r mean MAE: %r" % (c + mean[c]))
    best = min(cells, key=lambda c: (np.isnan(mean[c][0]), mean[c][0]))   # min() keeps the first of equal keys
    print("best: k %d mink %d mean RMSE %r" % (best + (mean[best][0],)))


def main(argv=None):
    args = parse_args(argv)
    users, items, ratings = read_ratings(args.input)
    weights = read_weights(args.weights) if args.weights else None
    if args.mode:
        from n2v_hip import eccstats
        weights = eccstats.item_statistics(users, items, ratings, args.windows, device=args.device).weights(args.mode)
    if args.save_weights:
        write_weights(args.save_weights, weights)
    if args.cv:
        results, maes = [], []
        for fold, (train, test) in enumerate(folds(len(ratings), args.cv, args.seed)):
            recs_path = "%s.%d" % (args.save_recs, fold) if args.save_recs else None
            result, mae = run_split(args, users, items, ratings, weights, train, test, recs_path)
            results.append(result)
            maes.append(mae)
            report(args, result, mae)
        if args.sweep_k is not None:
            report_sweep(args, results)
            return results
        print("mean RMSE: %r" % float(np.mean([r if args.topn is None else r[0] for r in results])))
        if args.mae:
            print("mean MAE: %r" % float(np.mean(maes)))
        return results
    train, test = split(len(ratings), args.test_ratio, args.seed)
    result, mae = run_split(args, users, items, ratings, weights, train, test, args.save_recs)
    report(args, result, mae)
    if args.sweep_k is not None:
        report_sweep(args, [result])
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
