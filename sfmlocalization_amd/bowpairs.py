"""The pair list of a map under construction from its views' BoW vectors: every view is paired with the k views nearest
to it in BoW space (sfmloc_bow_knn, include/sfmloc.h "All-views BoW k-NN": exact, all views in one call on the device),
and with its neighbours in the sequence.  The twin of bin/ComputeBoWPairs (csrc/bowpairs_cli.cpp): the same switches,
the same bytes.

    python -m sfmlocalization_amd.bowpairs -m <matchDir> [-k 20] [-v 0] [-w <window>] [--mutual]
                                           [-o <matchDir>/pairs.bow.txt] [--device 0] [--profile]

ExtFeatAndMatch chooses its view pairs in one of three ways: all V (V - 1) / 2 of them, the -v / -mf neighbours of a
video, which never pair a view with the same place seen on the way back, or a pair file (-p, hulo::readPairFile).  This
writes that file.  The workflow:

    ExtFeatAndMatch <matchDir> -sm                       features only
    TrainBoW <inputDir> <bowFile> [-p=pcaFile]           one <base>.bow per view
    python -m sfmlocalization_amd.bowpairs -m <matchDir> -k 20 -v 3
    ExtFeatAndMatch <matchDir> -p=<matchDir>/pairs.bow.txt

Views are those of <matchDir>/sfm_data.json ascending by id (as ExtFeatAndMatch orders them); a view's vector is
<matchDir>/<base>.bow, ravelled and converted to float32 as a query's is.  -v pairs every view with the next v views,
as ExtFeatAndMatch -v does, and those pairs are always kept; -w (default: the value of -v) keeps the k-NN from spending
k on them: row i's candidates are the views more than w places from i.  --mutual keeps a k-NN pair only if each view
lists the other.  One "a b" line per pair, a < b, ascending.
"""
import json
import os
import struct
import sys

import numpy as np

from . import extfeat, fileio

NAME = "ComputeBoWPairs"
USAGE = f"""Usage: {NAME}
[-m|--match_dir] the directory of sfm_data.json and the views' .bow vectors

[Optional]
[-k|--knn] neighbours per view (20)
[-v|--video_frame] pair every view with the next v views as well (0)
[-w|--window] the k-NN of view i looks only at views more than w places away (the value of -v)
[--mutual] keep a k-NN pair only if each view lists the other
[-o|--output_file] the pair file to write (default: pairs.bow.txt in the match directory)
[--device] HIP device (0)
[--profile] print the device milliseconds
"""


def knn_pairs(ids, nbr, count, video_frame=0, mutual=False):
    """The pairs (ids[min(i, j)], ids[max(i, j)]) for every j among the first count[i] entries of nbr[i] -- with `mutual`
    only where i is among row j's too -- united with extfeat.generate_video_match_pairs(ids, video_frame), which are
    always kept.  -> a list of (a, b), unique, ascending by (a, b).  ids: ascending view ids, one per row."""
    ids = [int(x) for x in ids]
    rows = [set(int(j) for j in np.asarray(nbr[i]).ravel()[:int(count[i])]) for i in range(len(ids))]
    pairs = set()
    for i, row in enumerate(rows):
        for j in row:
            if not mutual or i in rows[j]:
                pairs.add((ids[min(i, j)], ids[max(i, j)]))
    pairs.update((int(a), int(b)) for a, b in extfeat.generate_video_match_pairs(ids, int(video_frame)))
    return sorted(pairs)


def write_pair_file(path, pairs):
    """hulo::readPairFile's format (FileUtils.cpp:180-194): one "a b" line per pair"""
    with open(path, "w") as f:
        f.write("".join(f"{a} {b}\n" for a, b in pairs))


def run(match_dir, k=20, video_frame=0, window=None, mutual=False, out_file="pairs.bow.txt", device=0, profile=False,
        ops=None, log=print):
    """-> 0, or 1 with a message on stderr.  ops: the module whose bow_knn / bowknn_last_ms run (default: capi)"""
    sd_path = os.path.join(match_dir, "sfm_data.json")
    try:
        with open(sd_path) as f:
            views = extfeat._views(json.load(f), match_dir)
    except (OSError, ValueError, KeyError, TypeError) as e:
        print(f"{NAME}: {sd_path} cannot be read. ({e})", file=sys.stderr)
        return 1
    if len(views) < 2:
        print(f"{NAME}: {sd_path}: {len(views)} views (at least two)", file=sys.stderr)
        return 1
    rows, first = [], None
    for v in views:
        path = os.path.splitext(v["feat"])[0] + ".bow"
        if not os.path.isfile(path):
            print(f"{NAME}: {path}: no BoW vector of view {v['id']} (TrainBoW writes them)", file=sys.stderr)
            return 1
        try:
            vec = np.asarray(fileio.read_mat_bin(path)).ravel().astype(np.float32)
        except (OSError, ValueError, struct.error) as e:  # (struct.error: a file shorter than its header)
            print(f"{NAME}: {path} cannot be read. ({e})", file=sys.stderr)
            return 1
        if len(vec) == 0:
            print(f"{NAME}: {path}: an empty BoW vector", file=sys.stderr)
            return 1
        if rows and len(vec) != len(rows[0]):
            print(f"{NAME}: {path}: {len(vec)} values, {first} has {len(rows[0])}", file=sys.stderr)
            return 1
        first = first or path
        rows.append(vec)
    if ops is None:
        from . import capi as ops
    window = int(video_frame) if window is None else int(window)
    try:
        nbr, _, count = ops.bow_knn(np.stack(rows), int(k), window=window, device=device, profile=profile)
    except Exception as e:
        print(f"{NAME}: {getattr(e, 'message', e)}", file=sys.stderr)
        return 1
    pairs = knn_pairs([v["id"] for v in views], nbr, count, video_frame, mutual)
    path = out_file if os.path.isabs(out_file) else os.path.join(match_dir, out_file)
    try:
        write_pair_file(path, pairs)
    except OSError as e:
        print(f"{NAME}: {path} cannot be written. ({e})", file=sys.stderr)
        return 1
    log(f"BoW pairs: {len(pairs)} pairs of {len(views)} views (k {int(k)}, window {window}) -> {path}")
    if profile:
        log(f"device {ops.bowknn_last_ms():.3f} ms")
    return 0


def parse_args(argv):
    """-> the keyword arguments of run(), or None for a bad command line"""
    opt = {"-m": "", "-k": "20", "-v": "0", "-w": "", "-o": "pairs.bow.txt", "--device": "0"}
    long_names = {"--match_dir": "-m", "--knn": "-k", "--video_frame": "-v", "--window": "-w", "--output_file": "-o"}
    flags = {"--mutual": False, "--profile": False}
    i = 0
    while i < len(argv):
        a = argv[i]
        if a in flags:
            flags[a] = True
            i += 1
            continue
        if "=" in a and a.split("=", 1)[0] == "--device":
            a, val = a.split("=", 1)
        else:
            a = long_names.get(a, a)
            if a not in opt or i + 1 >= len(argv):
                return None
            val = argv[i + 1]
            i += 1
        opt[a] = val
        i += 1
    try:
        kw = dict(match_dir=opt["-m"], k=int(opt["-k"]), video_frame=int(opt["-v"]),
                  window=int(opt["-w"]) if opt["-w"] else None, out_file=opt["-o"], device=int(opt["--device"]),
                  mutual=flags["--mutual"], profile=flags["--profile"])
    except ValueError:
        return None
    if not kw["match_dir"] or not kw["out_file"] or kw["k"] < 1 or kw["video_frame"] < 0 or (kw["window"] or 0) < 0:
        return None
    return kw


def main(argv=None):
    kw = parse_args(sys.argv[1:] if argv is None else list(argv))
    if kw is None:
        sys.stderr.write(USAGE)
        return 1
    return run(log=lambda s: print(s, flush=True), **kw)


if __name__ == "__main__":
    sys.exit(main())
