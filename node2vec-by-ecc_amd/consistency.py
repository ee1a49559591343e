"""Drop-in for the working part of the reference's src/consistency.py: how item rarity, item eccentricity and user
eccentricity septiles move between two periods of a ratings file, and the per-user ie profile.

    python consistency.py -input ratings.csv (-first LO:HI -second LO:HI | -seg-point TW)
                          [-n 7] [-min-count 4] [-window-col timestamp|timewindow] [-device cuda:0]
                          [-out DIR] [-profile FILE.npy [-bins 100] [-weighted]]
                          [-features X.npy Y.npy [-item-emb emb.txt]]

The reference's script stops at names it never defines (calculate_all_schedl); what it is after is the three 7 x 7 tables
of src/utils.py:163-226 (septile_for_plot), whose heatmaps are only a rendering.  Here the tables are computed on the
device (n2v_hip.consistency) and printed; nothing is drawn.

-input       csv `user,item,rating,timestamp`, an optional header line is skipped
-first       the first period, an inclusive range of time windows LO:HI (an empty side is open); -second the second.
             The reference's MovieLens cut is  -first 201101:201298 -second 201301:201498
-seg-point   the reference's 30Music cut instead: windows <= TW against windows > TW
-n           bins per period (septiles: 7), at most 256;  -min-count  an item / user needs MORE rows than this in each period
-window-col  the 4th column is a unix timestamp, cut into UTC months (default), or the time window itself
-out         write ir_septile.csv, ie_septile.csv, ue_septile.csv there: `bin1,bin2,count,count_sum,ratio` lines, the
             reference's long tables
-profile     also write every user's ie profile (fp64 users x bins, .npy) and FILE.npy.users.txt with the uid of every row;
             -bins its bins (the reference: 100), -weighted the feedback share instead of the row share
-features    with -profile: the feature rows X (profile ++ item vector, or ++ the item's number) and their y = feedback;
             -item-emb a word2vec text file of item vectors (song2vec); rows whose item has none are dropped
"""
import argparse
import os

import numpy as np

FILES = {"ir": "ir_septile.csv", "ie": "ie_septile.csv", "ue": "ue_septile.csv"}


def parse_args(argv=None):
    from n2v_hip import consistency as C
    p = argparse.ArgumentParser(description="eccentricity consistency between two periods of a ratings file (HIP, gfx950)")
    p.add_argument("-input", required=True)
    p.add_argument("-first", default=None)
    p.add_argument("-second", default=None)
    p.add_argument("-seg-point", "-seg_point", dest="seg_point", type=int, default=None)
    p.add_argument("-n", type=int, default=7)
    p.add_argument("-min-count", dest="min_count", type=int, default=4)
    p.add_argument("-window-col", dest="window_col", default="timestamp", choices=["timestamp", "timewindow"])
    p.add_argument("-device", default="cuda:0")
    p.add_argument("-out", default=None)
    p.add_argument("-profile", default=None)
    p.add_argument("-bins", type=int, default=100)
    p.add_argument("-weighted", action="store_true")
    p.add_argument("-features", nargs=2, metavar=("X.npy", "Y.npy"), default=None)
    p.add_argument("-item-emb", dest="item_emb", default=None)
    a = p.parse_args(argv)
    if a.seg_point is not None:
        if a.first is not None or a.second is not None:
            p.error("-seg-point stands instead of -first / -second")
        a.periods = C.seg_point_intervals(a.seg_point)
    else:
        if a.first is None or a.second is None:
            p.error("give -first LO:HI and -second LO:HI, or -seg-point TW")
        try:
            a.periods = (C.parse_interval(a.first), C.parse_interval(a.second))
        except ValueError as e:
            p.error(str(e))
    if not 1 <= a.n <= C.MAX_BINS:
        p.error("-n must lie in 1 .. %d" % C.MAX_BINS)
    if not 1 <= a.bins <= C.MAX_BINS:
        p.error("-bins must lie in 1 .. %d" % C.MAX_BINS)
    if a.min_count < 0:
        p.error("-min-count must be at least 0")
    if a.features and not a.profile:
        p.error("-features needs -profile")
    if a.item_emb and not a.features:
        p.error("-item-emb belongs to -features")
    return a


def table_text(kind, table):
    """The ratio table as the heatmap shows it: one line per bin of the first period."""
    lines = ["%s: %d joined; rows: bin in the first period, columns: bin in the second" % (kind, len(table.ids))]
    for a, row in enumerate(table.ratio):
        lines.append("%3d  " % (a + 1) + " ".join("  nan" if v != v else "%5.2f" % v for v in row))
    return "\n".join(lines)


def frame_text(frame):
    lines = ["bin1,bin2,count,count_sum,ratio"]
    lines += ["%d,%d,%d,%d,%r" % (r.bin1, r.bin2, r.count, r.count_sum, float(r.ratio)) for r in frame]
    return "\n".join(lines) + "\n"


def main(a):
    import main_rec
    from n2v_hip import consistency as C
    users, items, ratings = main_rec.read_ratings(a.input)
    windows = main_rec.read_windows(a.input, a.window_col)
    res = C.transitions(users, items, ratings, windows, a.periods[0], a.periods[1], n=a.n, min_count=a.min_count, device=a.device)
    for kind in C.KINDS:
        print(table_text(kind, getattr(res, kind)))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        for kind in C.KINDS:
            with open(os.path.join(a.out, FILES[kind]), "w") as f:
                f.write(frame_text(res.frame(kind)))
    if a.profile:
        prof = C.user_ie_profile(users, items, ratings, windows, n_bins=a.bins, weighted=a.weighted, device=a.device)
        np.save(a.profile, prof.profile)
        with open(a.profile + ".users.txt", "w") as f:
            f.write("".join("%s\n" % u for u in prof.users))
        if a.features:
            vectors = None
            if a.item_emb:
                from n2v_hip import io as n2v_io
                words, vecs = n2v_io.load_word2vec_format(a.item_emb)
                vectors = {str(w): v for w, v in zip(words, np.asarray(vecs, dtype=np.float32))}
            X, y, _ = C.features(prof, users, items, ratings, item_vectors=vectors, device=a.device)
            np.save(a.features[0], X)
            np.save(a.features[1], y)
            print("features: %d rows x %d" % X.shape)
    return res


if __name__ == "__main__":
    main(parse_args())
