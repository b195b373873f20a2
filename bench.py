#!/usr/bin/env python3
"""Flagship benchmark: posts/sec, synthetic Telegram feed, GPU parse+encode.

BASELINE.json config #2 (scaled to N GPUs, weak scaling): per GPU, 1k
synthetic channels x 10k posts; the timed step runs the full per-post hot
path on one pre-generated device-resident chunk:

    HIP parse+encode (content switch, UTF-16 entity walk, t.me link
    extraction, Go-JSON line emission)
 -> seen-set claim (atomicCAS hash table) + bloom update
 -> cross-rank discovery exchange (all-gather of newly-claimed hashes,
    RCCL over xGMI) when world_size > 1
 -> D2H copy of the JSONL bytes into a pinned host ring (the storage
    binding boundary; --sink file additionally writes to disk)

Launch: python bench.py --gpus N --steps K --warmup W
(for N>1 the driver uses torch.distributed.run; RANK/LOCAL_RANK/WORLD_SIZE
are read from the env). Rank 0 prints ONE json line per the bench contract.

A plain run does only what the headline figure needs: setup, warmup,
priming, the K timed steps, the result line. --full adds the secondary
measurements (p50 single-channel latency, in-loop GPU-busy sampling);
their result fields are null without it. --dump-outputs DIR writes what
the last timed step produced as DIR/<name>.npy (see dump_outputs).
"""
import argparse
import datetime as dt
import json
import os
import statistics
import sys
import time

import numpy as np
import torch


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--channels", type=int, default=1000,
                    help="channels per GPU (flagship: 1000)")
    ap.add_argument("--posts", type=int, default=10000,
                    help="posts per channel (flagship: 10000)")
    ap.add_argument("--chunk-channels", type=int, default=125,
                    help="channels per device chunk (= step granularity)")
    ap.add_argument("--sink", choices=["pinned", "file", "none"],
                    default="pinned")
    ap.add_argument("--sink-dir", default="/tmp/crawl-bench")
    ap.add_argument("--platform", choices=["telegram", "youtube", "mixed"],
                    default="telegram",
                    help="mixed = even ranks telegram, odd ranks youtube "
                         "(BASELINE config #4 dispatch)")
    ap.add_argument("--videos", type=int, default=400_000,
                    help="videos per GPU for the youtube platform")
    ap.add_argument("--chunk-videos", type=int, default=100_000)
    ap.add_argument("--max-comments", type=int, default=1000,
                    help="accepted for CLI parity (the corpus knobs "
                         "below control the bench's comment shape)")
    ap.add_argument("--comment-rate", type=float, default=0.02,
                    help="telegram feed: fraction of posts with comment "
                         "threads (comment-heavy variant: 1.0)")
    ap.add_argument("--max-comments-per-post", type=int, default=3,
                    help="telegram feed: thread size cap (comment-heavy "
                         "variant: 250 exercises >100-comment posts)")
    ap.add_argument("--cpu", action="store_true",
                    help="debug: run the Python golden path on CPU (tiny)")
    ap.add_argument("--full", action="store_true",
                    help="also take the secondary measurements (p50 "
                         "single-channel latency, GPU-busy sampling)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs to "
                         "DIR/<name>.npy (float32/float64, <= 64 MB)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    if args.cpu:
        return run_cpu_debug(args)

    assert torch.cuda.is_available(), "bench requires a ROCm GPU"
    n_dev = torch.cuda.device_count()
    dev_idx = local_rank % n_dev
    if dev_idx != local_rank:
        log(f"rank {rank}: wrapping local_rank {local_rank} onto "
            f"cuda:{dev_idx} ({n_dev} visible devices — dry-run mode)")
    torch.cuda.set_device(dev_idx)
    device = torch.device("cuda", dev_idx)

    if world > 1:
        # CRAWL_BENCH_BACKEND=gloo lets a single-GPU box dry-run the
        # world>1 path (two ranks sharing cuda:0; collectives bounce
        # through CPU) before a real RCCL multi-GPU run
        torch.distributed.init_process_group(
            os.environ.get("CRAWL_BENCH_BACKEND", "nccl"))

    from crawler_amd.feed import FeedConfig, SyntheticFeed
    from crawler_amd.ops import gpu

    gpu.require_lib()

    # ---- setup (untimed): generate the per-rank corpus ----
    my_platform = args.platform
    if args.platform == "mixed":
        my_platform = "telegram" if rank % 2 == 0 else "youtube"

    chunks = []
    eff_channels = args.channels
    t_gen = time.time()
    if my_platform == "telegram":
        chunk_ch = args.chunk_channels
        posts = args.posts
        # keep each packed chunk's pools within int32 offsets: comment
        # threads inflate pool bytes/post (~60B per comment incl.
        # handles/reactions), so shrink the chunk until the estimate
        # fits ~1.6 GB (the flagship shape is unaffected: 203 B/post)
        est_post_bytes = 200
        if args.comment_rate > 0:
            est_post_bytes += int(args.comment_rate
                                  * (args.max_comments_per_post / 2 + 1)
                                  * 60)
        max_chunk_posts = max(posts, int(1.6e9 / est_post_bytes))
        if chunk_ch * posts > max_chunk_posts:
            chunk_ch = max(1, max_chunk_posts // posts)
            log(f"chunk_channels clamped to {chunk_ch} "
                f"({est_post_bytes} est pool B/post keeps int32 offsets)")
        channels = args.channels
        # the whole corpus stays resident in HBM across steps; cap it
        # so comment-heavy shapes fit the 288 GB card (weak scaling is
        # per-step, so fewer resident channels only shortens the cycle)
        max_total_posts = max(chunk_ch * posts,
                              int(200e9 / est_post_bytes))
        if channels * posts > max_total_posts:
            channels = max(chunk_ch, max_total_posts // posts)
            log(f"resident channels clamped to {channels} "
                f"(~{est_post_bytes * channels * posts / 1e9:.0f} GB "
                f"est pools fit HBM)")
        n_chunks = max(1, channels // chunk_ch)
        eff_channels = n_chunks * chunk_ch
        feed = SyntheticFeed(FeedConfig(
            seed=1234 + rank, universe=1_000_000,
            comment_rate=args.comment_rate,
            max_comments_per_post=args.max_comments_per_post))
        for c in range(n_chunks):
            ids = (np.arange(c * chunk_ch, (c + 1) * chunk_ch)
                   + rank * args.channels)
            chunks.append(
                feed.build_batch_device(ids, device, posts_per_channel=posts)
            )
            torch.cuda.synchronize()
            log(f"chunk {c + 1}/{n_chunks} generated on-device "
                f"({(c + 1) * chunk_ch * posts / 1e6:.2f}M posts, "
                f"{time.time() - t_gen:.1f}s)")
        chunk_posts = chunk_ch * posts
    else:
        from crawler_amd.youtube.batch import build_corpus_device
        from crawler_amd.youtube.synth import SyntheticYouTubeIndex

        idx = SyntheticYouTubeIndex(seed=99 + rank,
                                    universe_channels=1_000_000)
        n_chunks = max(1, args.videos // args.chunk_videos)
        for c in range(n_chunks):
            # device-side generation (yt_feedgen.hip) — the corpus
            # never leaves HBM, like the telegram feedgen path
            chunks.append(
                build_corpus_device(idx, args.chunk_videos, device,
                                    crawl_label="yt-bench")
            )
            log(f"yt chunk {c + 1}/{n_chunks} "
                f"({args.chunk_videos} videos, "
                f"{time.time() - t_gen:.1f}s)")
        chunk_posts = args.chunk_videos

    now = dt.datetime(2026, 1, 1, tzinfo=dt.timezone.utc)
    seen = gpu.SeenSet(device)

    # Double-buffered pinned host ring for the JSONL output (the storage
    # boundary): D2H of step k overlaps the kernels of step k+1 on a
    # separate copy stream. Worst case ~2.6KB/post.
    host_alloc_state = {"pinned": True}

    def alloc_host(nbytes):
        # 8 ranks x 2 buffers of pinned memory can brush against host
        # lockable-memory limits; fall back to pageable rather than fail
        # — but RECORD it (result JSON carries pinned per rank: a
        # pageable fallback silently changes what is measured)
        try:
            return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        except RuntimeError:
            host_alloc_state["pinned"] = False
            print(f"[bench rank{rank}] pinned allocation failed; "
                  "using pageable host memory", file=sys.stderr, flush=True)
            return torch.empty(nbytes, dtype=torch.uint8)

    # worst-case line sizes differ by platform: telegram ~2.1KB/post,
    # youtube ~3.0KB/video (richer channel block per line). Comment
    # threads add ~230B per comment (avg thread = half the cap) — the
    # ring assert below catches any underestimate loudly.
    per_post = 2600 if my_platform == "telegram" else 3600
    if my_platform == "telegram" and args.comment_rate > 0:
        avg_thread = args.max_comments_per_post / 2 + 1
        per_post += int(args.comment_rate * avg_thread * 230 * 1.4)
    pinned = [alloc_host(int(chunk_posts * per_post)) for _ in range(2)]
    compute_stream = torch.cuda.Stream()
    # two copy streams: MI355X has multiple SDMA engines; splitting the
    # 2.5GB D2H in half across streams uses two of them
    copy_streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    n_copy = 2 if os.environ.get("CRAWL_ONE_SDMA", "") != "1" else 1
    inflight = [None, None]  # keep res tensors alive while copying
    sink_f = None
    if args.sink == "file":
        # rank-sharded sink files: every rank writes its own shard so
        # an 8-rank file-sink run measures true aggregate disk pressure
        os.makedirs(args.sink_dir, exist_ok=True)
        sink_f = open(os.path.join(args.sink_dir, f"rank{rank}.jsonl"), "wb")

    total_out_bytes = 0
    new_discoveries = 0
    # --dump-outputs: what the last timed step handed to its caller
    last_si = args.warmup + args.steps - 1
    last_out = {}

    def step(si):
        nonlocal total_out_bytes, new_discoveries
        chunk = chunks[si % n_chunks]
        slot = si % 2
        with torch.cuda.stream(compute_stream):
            if my_platform == "telegram":
                res = gpu.parse_encode(
                    chunk, now=now,
                    single_pass=os.environ.get("CRAWL_SINGLE_PASS", "") == "1",
                )
                out_t = res.out
                new_mask = seen.claim(res)
                if world > 1:
                    # count-sized exchange + bloom OR-union — no cap
                    # (round 1 silently truncated at 64k hashes/step)
                    flat = new_mask.flatten().bool()
                    new_hashes = res.link_hash.flatten()[flat]
                    seen.merge_remote(new_hashes, torch.distributed,
                                      world)
                nd = seen.new_count()  # syncs within the compute stream
                if args.dump_outputs and si == last_si:
                    last_out.update(
                        line_off=res.line_off, line_len=res.line_len,
                        link_cnt=res.link_cnt, link_hash=res.link_hash)
            else:
                out_t, _off, _len = gpu.yt_parse_encode(chunk, now=now)
                if args.dump_outputs and si == last_si:
                    last_out.update(line_off=_off, line_len=_len)
                if world > 1:
                    # mixed dispatch still exchanges (empty) discovery
                    # buffers so collectives stay symmetric across ranks
                    empty = torch.zeros(0, dtype=torch.int64,
                                        device=device)
                    seen.merge_remote(empty, torch.distributed, world)
                nd = 0
        nbytes = out_t.numel()
        assert nbytes <= pinned[slot].numel(), (
            f"host ring too small: {nbytes} > {pinned[slot].numel()}"
        )
        ev = torch.cuda.Event()
        ev.record(compute_stream)
        # the previous copy into this pinned slot must be done before reuse
        if inflight[slot] is not None:
            for d in inflight[slot][1]:
                d.synchronize()
        dones = []
        half = (nbytes // n_copy + 15) & ~15
        for ci in range(n_copy):
            cs = copy_streams[ci]
            cs.wait_event(ev)
            lo = ci * half
            hi = min(nbytes, lo + half)
            if lo >= hi:
                continue
            with torch.cuda.stream(cs):
                pinned[slot][lo:hi].copy_(out_t[lo:hi], non_blocking=True)
                out_t.record_stream(cs)
            d = torch.cuda.Event()
            d.record(cs)
            dones.append(d)
        inflight[slot] = (out_t, dones)
        total_out_bytes += nbytes
        new_discoveries += nd
        if args.dump_outputs and si == last_si:
            last_out.update(jsonl=pinned[slot][:nbytes], new_discoveries=nd)
        if sink_f is not None:
            for d in dones:
                d.synchronize()
            sink_f.write(bytes(pinned[slot][:nbytes].numpy()))
        return nbytes

    # ---- warmup ----
    for w in range(args.warmup):
        step(w)
    log(f"warmup done ({args.warmup} steps)")

    # ---- p50 channel latency (BASELINE secondary metric): one channel's
    # batch through the full pipeline (parse+encode -> claim -> D2H) ----
    p50_channel_ms = None
    if args.full and my_platform == "telegram":
        lat = []
        one = feed.build_batch_device(
            np.array([999_990 + rank]), device, posts_per_channel=args.posts
        )
        lat_pin = alloc_host(args.posts * (per_post + 400))
        for _ in range(11):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r1 = gpu.parse_encode(one, now=now)
            seen.claim(r1)
            lat_pin[: r1.out.numel()].copy_(r1.out, non_blocking=True)
            torch.cuda.synchronize()
            lat.append((time.perf_counter() - t) * 1000)
        p50_channel_ms = round(statistics.median(lat), 3)
        log(f"p50 channel latency: {p50_channel_ms} ms "
            f"({args.posts} posts/channel)")

    # Untimed priming IMMEDIATELY before the timed region: a
    # freshly-idle MI355X starts at low DVFS clocks, and clocks decay
    # within the idle gaps of setup/p50 measurement — short runs (small
    # --steps) would otherwise under-read by ~2x while the first timed
    # steps re-ramp. This only loads the compute pipeline (no claims,
    # no D2H side effects); the timed region is unchanged.
    t_pr = time.time()
    prim = 0
    while time.time() - t_pr < 3.0 and prim < 60:
        if my_platform == "telegram":
            gpu.parse_encode(chunks[0], now=now)
        else:
            gpu.yt_parse_encode(chunks[0], now=now)
        torch.cuda.synchronize()
        prim += 1
    log(f"primed {prim} iterations ({time.time() - t_pr:.1f}s)")

    # ---- timed region ----
    # In-loop GPU-busy sampling (sysfs gpu_busy_percent, ~50 ms cadence)
    # so short runs carry their own utilization record — a single
    # post-hoc SMI sample can miss a 5 s run entirely.
    import glob as _glob
    import threading as _threading
    busy_samples = []
    stop_busy = _threading.Event()
    busy_paths = sorted(_glob.glob(
        "/sys/class/drm/card*/device/gpu_busy_percent"))
    if not args.full:
        busy_paths = []  # secondary measurement: sampler never starts

    def _busy_sampler():
        while not stop_busy.is_set():
            for p in busy_paths:
                try:
                    with open(p) as f:
                        busy_samples.append(int(f.read().strip()))
                except (OSError, ValueError):
                    pass
            stop_busy.wait(0.05)

    sampler = _threading.Thread(target=_busy_sampler, daemon=True)

    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    if busy_paths:
        sampler.start()
    step_times = []
    t0 = time.perf_counter()
    for si in range(args.steps):
        ts = time.perf_counter()
        step(args.warmup + si)
        step_times.append((time.perf_counter() - ts) * 1000)
    torch.cuda.synchronize()
    stop_busy.set()
    if world > 1:
        torch.distributed.barrier()
    t1 = time.perf_counter()

    elapsed = t1 - t0
    if world > 1:
        e = torch.tensor([elapsed], device=device)
        torch.distributed.all_reduce(e, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(e.item())

    # per-rank hygiene record: pinned-or-pageable + achieved D2H GB/s
    # (JSONL bytes moved device->host inside the timed region / elapsed)
    timed_bytes = args.steps * (total_out_bytes
                                // max(1, args.warmup + args.steps))
    my_d2h_gbs = timed_bytes / elapsed / 1e9
    if world > 1:
        info = torch.tensor(
            [1.0 if host_alloc_state["pinned"] else 0.0, my_d2h_gbs],
            device=device)
        g_info = [torch.empty_like(info) for _ in range(world)]
        torch.distributed.all_gather(g_info, info)
        per_rank_host = [
            {"pinned": bool(g[0].item() > 0.5),
             "d2h_gbs": round(float(g[1].item()), 2)}
            for g in g_info
        ]
    else:
        per_rank_host = [{"pinned": host_alloc_state["pinned"],
                          "d2h_gbs": round(my_d2h_gbs, 2)}]

    posts_done = args.steps * chunk_posts
    if world > 1:
        # whole-job aggregate: SUM the per-rank work (ranks differ in
        # --platform mixed, where telegram and youtube step sizes differ)
        pd = torch.tensor([float(posts_done)], device=device)
        torch.distributed.all_reduce(pd)  # default op = SUM
        total_done = float(pd.item())
    else:
        total_done = float(posts_done)
    value = total_done / elapsed

    if sink_f is not None:
        sink_f.close()

    if args.dump_outputs and rank == 0 and last_out:
        # after the timed region's final synchronize: the host ring slot
        # and the device tensors of the last step are complete
        dump_outputs(args.dump_outputs, last_out)

    if rank == 0:
        result = {
            "metric": "posts/sec (whole node) synthetic feed",
            "value": round(value, 1),
            "unit": "posts/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed * 1000 / args.steps, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "uint8",
            "data": "synthetic",
            "config": {
                "model": ("telegram-crawl 1k-channels x 10k-posts per GPU "
                          "(BASELINE config #2, weak-scaled)"
                          if args.platform == "telegram" else
                          f"{args.platform} crawl (BASELINE config #4 dispatch)"),
                "global_batch": int(total_done / args.steps),
                "seq_len": 0,
                "platform": args.platform,
                "parallelism": f"dp{world} (channel-sharded, RCCL discovery "
                               "all-gather)" if world > 1 else "dp1",
                "channels_per_gpu": eff_channels,
                "posts_per_channel": args.posts,
                "chunk_posts": chunk_posts,
                "jsonl_bytes_per_step": total_out_bytes // max(
                    1, args.warmup + args.steps),
                "p50_step_ms": round(statistics.median(step_times), 2),
                "p50_channel_latency_ms": p50_channel_ms,
                "new_discoveries": new_discoveries,
                "sink": args.sink,
                "pinned": all(r["pinned"] for r in per_rank_host),
                "per_rank_host": per_rank_host,
                "gpu_busy_sampled": (
                    {"mean": round(sum(busy_samples) / len(busy_samples),
                                   1),
                     "max": max(busy_samples),
                     "n": len(busy_samples)}
                    if busy_samples else None),
                "comment_rate": args.comment_rate,
                "max_comments_per_post": args.max_comments_per_post,
            },
        }
        print(json.dumps(result), flush=True)

    if world > 1:
        torch.distributed.destroy_process_group()


DUMP_SEED = 20260101
DUMP_MAX_ROWS = 1_250_000       # per-row arrays: one flagship step, whole
DUMP_HASH_ROWS = 65_536
DUMP_WINDOWS, DUMP_WINDOW = 128, 32_768
DUMP_BLOCK = 1 << 20


def dump_outputs(dirpath, last):
    """Write the last timed step's outputs as float32/float64 .npy files.

    The step hands its caller the JSONL bytes in the host ring plus the
    per-post line table and extracted links; a flagship step is 2.5 GB
    of JSONL, so the files stay under 64 MB in all by sampling with a
    fixed seed (same arguments -> same inputs, rows and windows):

      jsonl_block_sums  f64  sum of every 1 MiB block of the JSONL bytes
                             (covers every byte), last entry = tail
      jsonl_sample      f32  128 seeded 32 KiB windows of the JSONL bytes
                             (all bytes if the output is smaller)
      line_off          f64  per post: every post of a step of up to
      line_len          f32  DUMP_MAX_ROWS, else a seeded sorted row sample
      link_cnt          f32  (telegram) same rows
      link_hash         f64  (telegram) [rows, MAX_LINKS, 2] = high and
                             low 32 bits of the fnv1a64 link hashes, for
                             a seeded sample of DUMP_HASH_ROWS posts
      new_discoveries   f64  [1] first-time links claimed by the step

    The per-link new_mask is left out: which of two posts carrying the
    same new link wins the atomicCAS claim is a race; the count is not.
    """
    os.makedirs(dirpath, exist_ok=True)

    def save(name, arr):
        assert arr.dtype in (np.float32, np.float64)
        np.save(os.path.join(dirpath, name + ".npy"), arr)
        return arr.nbytes

    def rows_of(n, cap):
        if n <= cap:
            return None
        rng = np.random.default_rng([DUMP_SEED, cap])
        return np.sort(rng.choice(n, size=cap, replace=False))

    def take(t, rows):
        if rows is not None:
            t = t[torch.from_numpy(rows).to(t.device)]
        return t.cpu().numpy()

    total = 0
    jsonl = last["jsonl"].numpy()
    nbytes = jsonl.shape[0]
    nblk = nbytes // DUMP_BLOCK
    sums = jsonl[:nblk * DUMP_BLOCK].reshape(nblk, DUMP_BLOCK).sum(
        axis=1, dtype=np.uint64).astype(np.float64)
    tail = np.float64(jsonl[nblk * DUMP_BLOCK:].sum(dtype=np.uint64))
    total += save("jsonl_block_sums", np.append(sums, tail))
    if nbytes <= DUMP_WINDOWS * DUMP_WINDOW:
        sample = jsonl
    else:
        rng = np.random.default_rng(DUMP_SEED)
        starts = np.sort(rng.integers(0, nbytes - DUMP_WINDOW,
                                      size=DUMP_WINDOWS))
        sample = np.concatenate([jsonl[s:s + DUMP_WINDOW] for s in starts])
    total += save("jsonl_sample", sample.astype(np.float32))

    n = last["line_len"].shape[0]
    rows = rows_of(n, DUMP_MAX_ROWS)
    total += save("line_off", take(last["line_off"], rows).astype(np.float64))
    total += save("line_len", take(last["line_len"], rows).astype(np.float32))
    if "link_cnt" in last:
        total += save("link_cnt",
                      take(last["link_cnt"], rows).astype(np.float32))
        h = take(last["link_hash"], rows_of(n, DUMP_HASH_ROWS))
        h = np.ascontiguousarray(h).view(np.uint64)
        total += save("link_hash", np.stack(
            [(h >> np.uint64(32)).astype(np.float64),
             (h & np.uint64(0xFFFFFFFF)).astype(np.float64)], axis=-1))
    total += save("new_discoveries",
                  np.array([last["new_discoveries"]], dtype=np.float64))
    assert total <= 64_000_000, f"dump is {total} bytes"
    log(f"dumped last-step outputs to {dirpath} ({total / 1e6:.1f} MB)")


def run_cpu_debug(args):
    """Tiny CPU sanity run of the same pipeline via the golden encoder."""
    from crawler_amd.feed import FeedConfig, SyntheticFeed
    from crawler_amd.ops.golden_batch import encode_batch

    feed = SyntheticFeed(FeedConfig(seed=1234, universe=10_000))
    batch = feed.build_batch(np.arange(4), posts_per_channel=100)
    now = dt.datetime(2026, 1, 1, tzinfo=dt.timezone.utc)
    t0 = time.perf_counter()
    lines, links = encode_batch(batch, now=now)
    dt_s = time.perf_counter() - t0
    print(json.dumps({
        "metric": "posts/sec (cpu golden debug)",
        "value": round(batch.n / dt_s, 1),
        "unit": "posts/s",
        "n_gpus": 0,
        "bytes": sum(len(l) for l in lines),
        "links": sum(len(l) for l in links),
    }))


if __name__ == "__main__":
    main()
