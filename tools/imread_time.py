"""What decoding a query JPEG costs on each route, per frame (needs a GPU and Pillow; writes profiles/imread_time.json):

    python tools/imread_time.py [--out profiles/imread_time.json] [--rounds 30]

Frames: a 640 x 480 and a 1920 x 1080 view of an imageworld, written as 4:2:0 JPEGs at quality 90.
  (a) host route       sfmloc_image_decode gray + colour, one host core (what a tool with a BoW shortlist pays today),
                       and each read alone
  (b) device route, host side   header + ONE entropy pass + staging (sfmloc_imread_timing)
  (c) device route, device side upload, IDCT launch, upsampling + colour launch by events; the whole decode call to
                       completion by a host clock around decode + the wait for its last event
  (d) frame to pose    from JPEG bytes for a frame alone, VGA, on the map of tests/test_gpu_image_in.py's scale:
                       host gray decode -> detect_resident -> localise  against  device decode -> detect_resident_dev ->
                       localise, alternating in one process; the results must be the same bits
Medians and minima over the rounds after a warm-up; the two routes alternate inside every round."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import imageworld  # noqa: E402
import sfmlocalization_amd as S  # noqa: E402
from sfmlocalization_amd import capi  # noqa: E402


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4)}


def jpeg_420_q90(gray):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.stack([gray, gray, gray], 2)).save(b, "JPEG", quality=90, subsampling=2)
    return b.getvalue()


def time_decode(data, rounds):
    w, h = (int(v) for v in S.image_decode(data).shape[::-1])
    r = capi.DeviceImread(w, h)
    r.timing(True)
    out = {"width": w, "height": h, "jpeg_bytes": len(data)}
    host = {"gray": [], "colour": [], "gray_plus_colour": []}
    dev = {m: {"host": [], "upload": [], "idct": [], "upsample_colour": [], "call_to_completion": []}
           for m in ("GRAY", "GRAY|BGR", "BGR2GRAY")}
    masks = {"GRAY": capi.IMREAD_GRAY, "GRAY|BGR": capi.IMREAD_GRAY | capi.IMREAD_BGR, "BGR2GRAY": capi.IMREAD_BGR2GRAY}
    for it in range(rounds + 3):
        t0 = time.perf_counter()
        S.image_decode(data, color=False)
        t1 = time.perf_counter()
        S.image_decode(data, color=True)
        t2 = time.perf_counter()
        if it >= 3:
            host["gray"].append((t1 - t0) * 1e3)
            host["colour"].append((t2 - t1) * 1e3)
            host["gray_plus_colour"].append((t2 - t0) * 1e3)
        for name, mask in masks.items():
            t0 = time.perf_counter()
            r.decode(data, mask)
            # (the timing call waits for the decode's last event)
            hp, up, idct, col = r.timing(True, read=True)
            t1 = time.perf_counter()
            if it >= 3:
                d = dev[name]
                d["host"].append(hp)
                d["upload"].append(up)
                d["idct"].append(idct)
                d["upsample_colour"].append(col)
                d["call_to_completion"].append((t1 - t0) * 1e3)
    r.close()
    out["host_route"] = {k: stats(v) for k, v in host.items()}
    out["device_route"] = {m: {k: stats(v) for k, v in d.items()} for m, d in dev.items()}
    g = dev["GRAY|BGR"]
    blocks = ((w + 15) // 16) * ((h + 15) // 16) * 6
    out["blocks_420"] = blocks
    out["upload_bytes_gray_bgr"] = 1024 + blocks * 128
    out["kernels_over_entropy_pass"] = round((statistics.median(g["idct"]) + statistics.median(g["upsample_colour"])) /
                                             statistics.median(g["host"]), 4)
    out["host_time_moved_fraction"] = round(1.0 - statistics.median(g["host"]) / statistics.median(host["gray_plus_colour"]), 4)
    return out


def frame_to_pose(rounds):
    W, H = 640, 480
    w = imageworld.build(S, 5, 36, 6, tiles=2, n_pad_views=30, pad_desc_per_view=500)
    m = w.m
    files = [jpeg_420_q90(f) for f in w.frames]
    res = {"frames": len(files), "map_views": int(len(m.view_id)), "map_rows": int(len(m.desc))}
    with S.Map(m.view_id, m.view_off, m.desc, params=S.default_params(ransac_round=25), view_wh=m.view_wh, kpt_xy=m.kpt_xy,
               row_landmark=m.row_landmark, landmark_id=m.landmark_id, landmark_X=m.landmark_X, intrinsic=m.intrinsic) as dm:
        ctx = dm.context()
        ak = S.Akaze(W, H)
        ak.share_stream(ctx)
        rd = capi.DeviceImread(W, H)
        rd.share_stream(ctx)

        def host_route(data):
            gray = S.image_decode(data, color=False)
            n = ak.detect_resident(gray)
            q = ak.query_view(dm, n)
            ctx.begin(q)
            got = ctx.end()
            q.close()
            return got

        def device_route(data):
            rd.decode(data, capi.IMREAD_GRAY)
            n = ak.detect_resident_dev(rd, capi.IMREAD_GRAY)
            q = ak.query_view(dm, n)
            ctx.begin(q)
            got = ctx.end()
            q.close()
            return got

        t_host, t_dev, same, ok = [], [], True, 0
        for it in range(rounds + 2):
            for data in files:
                t0 = time.perf_counter()
                a = host_route(data)
                t1 = time.perf_counter()
                b = device_route(data)
                t2 = time.perf_counter()
                same = same and capi.result_fingerprint(*a) == capi.result_fingerprint(*b)
                if it >= 2:
                    t_host.append((t1 - t0) * 1e3)
                    t_dev.append((t2 - t1) * 1e3)
                    ok += int(b[0].ok)
        rd.close()
        ak.close()
    res["host_decode_route"] = stats(t_host)
    res["device_decode_route"] = stats(t_dev)
    res["results_identical"] = bool(same)
    res["localised_fraction"] = round(ok / max(1, len(t_dev)), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imread_time.json"))
    ap.add_argument("--rounds", type=int, default=30)
    a = ap.parse_args()
    if S.device_count() < 1:
        raise SystemExit("imread_time: needs a HIP device (a time taken without one says nothing)")
    import torch
    atlas = imageworld.make_atlas(7, 2, 1600, torch.device("cuda", 0))
    rng = np.random.Generator(np.random.PCG64(7))
    Rs, Cs = imageworld.cameras(rng, 1, (0.0, 0.0), 16.0)
    out = {"rounds": a.rounds, "frames": {}}
    for name, (w, h, focal) in (("640x480", (640, 480, 800.0)), ("1920x1080", (1920, 1080, 2400.0))):
        frame = imageworld.render(atlas, 100.0, Rs, Cs, focal, w, h)[0]
        out["frames"][name] = time_decode(jpeg_420_q90(frame), a.rounds)
    del atlas
    out["frame_to_pose_vga"] = frame_to_pose(max(3, a.rounds // 3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
