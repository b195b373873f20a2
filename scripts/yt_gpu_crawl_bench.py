#!/usr/bin/env python
"""End-to-end rate of the YouTube GPU crawl mode, disk included.

Runs random sampling through youtube/gpu_runner.run_youtube_gpu at
--limit videos (quota lifted, max_searches high enough to reach it) and
the CPU youtube/runner.run_youtube with the same flags at --cpu-limit
(the CPU path does ~700 videos/s, so the full size would take tens of
minutes). Prints videos/s for both and the GPU run's split: sampling
rounds, generate+encode, D2H, file fan-out.

    python scripts/yt_gpu_crawl_bench.py --limit 1000000 --cpu-limit 10000
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
    ap.add_argument("--storage-root", default="",
                    help="default: a temporary directory, removed after")
    args = ap.parse_args(argv)

    import torch

    from crawler_amd.config import CrawlerConfig
    from crawler_amd.youtube.gpu_runner import run_youtube_gpu
    from crawler_amd.youtube.runner import run_youtube

    root = args.storage_root or tempfile.mkdtemp(prefix="yt-gpu-bench-")
    big = 10 ** 15

    def cfg(crawl_id, limit):
        # ~1.6 verified videos per search: 2x headroom on the searches
        return CrawlerConfig(
            storage_root=root, crawl_id=crawl_id, platform="youtube",
            sampling_method="random", max_posts=limit, crawl_label="bench",
            synthetic_seed=args.seed, yt_max_searches=2 * limit + 1000,
            yt_daily_quota=big)

    try:
        # warm the runtime (library load, allocator) outside the timing
        run_youtube_gpu(cfg("warm", 256), [], round_searches=256)
        timings = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = run_youtube_gpu(cfg("gpu", args.limit), [],
                                round_searches=args.round_searches,
                                timings=timings)
        wall = time.perf_counter() - t0
        split = {k: round(timings[k], 4)
                 for k in ("sample", "gen_encode", "d2h", "fanout")}
        out = {
            "mode": "gpu", "limit": args.limit,
            "videos": stats["videos"], "searches": stats["searches"],
            "wall_s": round(wall, 4),
            "videos_per_s": round(stats["videos"] / wall, 1),
            "split_s": split,
            "jsonl_bytes": timings.get("jsonl_bytes", 0),
            "d2h_gbs": round(timings.get("jsonl_bytes", 0)
                             / max(timings["d2h"], 1e-9) / 1e9, 3),
            "claim_grown": timings.get("claim_grown", 0),
        }
        print(json.dumps(out), flush=True)
        if args.cpu_limit > 0:
            t0 = time.perf_counter()
            cstats = run_youtube(cfg("cpu", args.cpu_limit), [])
            cwall = time.perf_counter() - t0
            print(json.dumps({
                "mode": "cpu", "limit": args.cpu_limit,
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
