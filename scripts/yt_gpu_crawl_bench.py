#!/usr/bin/env python
"""End-to-end rate of the YouTube GPU crawl mode, disk included.

Runs random (default) or snowball sampling through
youtube/gpu_runner.run_youtube_gpu at --limit videos (quota lifted,
max_searches high enough to reach it) and the CPU
youtube/runner.run_youtube with the same flags at --cpu-limit (the CPU
path does ~700 videos/s, so the full size would take tens of minutes).
Prints videos/s for both and the GPU run's split: sampling (search rounds
or snowball layers), generate+encode, D2H, file fan-out.

    python scripts/yt_gpu_crawl_bench.py --limit 1000000 --cpu-limit 10000
    python scripts/yt_gpu_crawl_bench.py --sampling snowball \
        --seeds 99,33,150 --max-depth 6 --limit 1000000 --cpu-limit 10000
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--limit", type=int, default=1_000_000)
    ap.add_argument("--cpu-limit", type=int, default=10_000,
                    help="0 skips the CPU run")
    ap.add_argument("--seed", type=int, default=99)
    ap.add_argument("--round-searches", type=int, default=65536)
    ap.add_argument("--sampling", choices=["random", "snowball"],
                    default="random")
    ap.add_argument("--seeds", default="99,33,150",
                    help="snowball: comma-separated seed channel indices")
    ap.add_argument("--max-depth", type=int, default=6,
                    help="snowball: BFS depth")
    ap.add_argument("--snowball-steps", action="store_true",
                    help="snowball: also time the layer loop's steps "
                         "(a device synchronisation per step)")
    ap.add_argument("--storage-root", default="",
                    help="default: a temporary directory, removed after")
    args = ap.parse_args(argv)

    import torch

    from crawler_amd.config import CrawlerConfig
    from crawler_amd.youtube.gpu_runner import run_youtube_gpu
    from crawler_amd.youtube.runner import run_youtube

    root = args.storage_root or tempfile.mkdtemp(prefix="yt-gpu-bench-")
    big = 10 ** 15
    urls = ([u for u in args.seeds.split(",") if u]
            if args.sampling == "snowball" else [])

    def cfg(crawl_id, limit):
        # ~1.6 verified videos per search: 2x headroom on the searches
        return CrawlerConfig(
            storage_root=root, crawl_id=crawl_id, platform="youtube",
            sampling_method=args.sampling, max_posts=limit,
            max_depth=args.max_depth, crawl_label="bench",
            synthetic_seed=args.seed, yt_max_searches=2 * limit + 1000,
            yt_daily_quota=big)

    try:
        # warm the runtime (library load, allocator) outside the timing
        run_youtube_gpu(cfg("warm", 256), urls, round_searches=256)
        timings = {}
        if args.sampling == "snowball" and args.snowball_steps:
            timings["snowball_steps"] = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = run_youtube_gpu(cfg("gpu", args.limit), urls,
                                round_searches=args.round_searches,
                                timings=timings)
        wall = time.perf_counter() - t0
        split = {k: round(timings[k], 4)
                 for k in ("sample", "gen_encode", "d2h", "fanout")}
        out = {
            "mode": "gpu", "sampling": args.sampling, "limit": args.limit,
            "videos": stats["videos"], "searches": stats["searches"],
            "video_batches": stats["video_batches"],
            "layers": timings.get("snowball_layers", 0),
            "wall_s": round(wall, 4),
            "videos_per_s": round(stats["videos"] / wall, 1),
            "split_s": split,
            "jsonl_bytes": timings.get("jsonl_bytes", 0),
            "d2h_gbs": round(timings.get("jsonl_bytes", 0)
                             / max(timings["d2h"], 1e-9) / 1e9, 3),
            "claim_grown": timings.get("claim_grown", 0),
        }
        if "snowball_steps" in timings:
            out["sample_steps_s"] = {k: round(v, 4) for k, v in
                                     timings["snowball_steps"].items()}
        print(json.dumps(out), flush=True)
        if args.cpu_limit > 0:
            t0 = time.perf_counter()
            cstats = run_youtube(cfg("cpu", args.cpu_limit), urls)
            cwall = time.perf_counter() - t0
            print(json.dumps({
                "mode": "cpu", "sampling": args.sampling,
                "limit": args.cpu_limit,
                "videos": cstats["videos"],
                "searches": cstats["searches"],
                "wall_s": round(cwall, 4),
                "videos_per_s": round(cstats["videos"] / cwall, 1),
            }), flush=True)
    finally:
        if not args.storage_root:
            shutil.rmtree(root, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
