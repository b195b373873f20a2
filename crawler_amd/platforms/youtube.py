"""YouTube platform crawler plugin.

Parity: crawler/youtube/youtube_crawler.go (sampling dispatch,
conversion pool) behind the registry interface of crawler/crawler.go.
"""
from __future__ import annotations

import sys

from ..registry import CrawlContext, PlatformCrawler


class YouTubeCrawler(PlatformCrawler):
    def platform_type(self) -> str:
        return "youtube"

    def run(self, ctx: CrawlContext) -> dict:
        from ..youtube.runner import run_youtube

        if getattr(ctx.args, "gpu", False):
            method = ctx.cfg.sampling_method
            if method in ("random", "channel") or (
                    method == "snowball"
                    and getattr(ctx.args, "yt_gpu_snowball", False)):
                from ..youtube.gpu_runner import run_youtube_gpu

                stats = run_youtube_gpu(ctx.cfg, ctx.urls)
                print(f"youtube gpu crawl complete: {stats}",
                      file=sys.stderr)
                return stats
            print("youtube: the GPU mode covers random and channel "
                  "sampling; running snowball on the CPU "
                  "(--yt-gpu-snowball runs it on the GPU)",
                  file=sys.stderr)
        stats = run_youtube(ctx.cfg, ctx.urls)
        print(f"youtube crawl complete: {stats}", file=sys.stderr)
        return stats


def register(registry) -> None:
    registry.register("youtube", YouTubeCrawler)
