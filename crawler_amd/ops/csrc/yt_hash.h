// The synthetic YouTube index on the device (youtube/synth.py
// SyntheticYouTubeIndex): its splitmix64 hash chains, the id and
// channel-meta derivations built on them, and the launch-grid helper.
// Shared by the generator (yt_feedgen.hip), the sampling kernels
// (yt_sample.hip) and snowball discovery (yt_snowball.hip).
#pragma once

#include "common.h"

namespace crawl {

DEV unsigned long long yt_smx(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

__device__ const char YT_ALPH[64 + 1] =
    "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-_";

// scalar _h prefix chain over a constant string
DEV unsigned long long yt_chain(unsigned long long a, const char* s) {
  for (; *s; ++s) a = yt_smx(a ^ (unsigned long long)(unsigned char)*s);
  return a;
}

// the index's hash base: every _h chain starts from it
DEV unsigned long long yt_base(long long seed) {
  return (unsigned long long)seed ^ 0xC0FFEEULL;
}

// video_id(prefix, k): prefix + '-' + 5 hash chars
DEV void yt_video_id(unsigned long long base, const unsigned char* pc,
                     unsigned long long k, unsigned char* vid) {
  unsigned long long a = yt_chain(base, "vid");
  for (int j = 0; j < 5; ++j) a = yt_smx(a ^ (unsigned long long)pc[j]);
  unsigned long long h1 = yt_smx(a ^ k);
  for (int j = 0; j < 5; ++j) vid[j] = pc[j];
  vid[5] = '-';
  for (int j = 0; j < 5; ++j)
    vid[6 + j] = (unsigned char)YT_ALPH[(h1 >> (6 * j)) % 64ULL];
}

// _h("vidmeta", id): every per-video field derives from it
DEV unsigned long long yt_vidmeta_hash(unsigned long long base,
                                       const unsigned char* vid) {
  unsigned long long a = yt_chain(base, "vidmeta");
  for (int j = 0; j < 11; ++j) a = yt_smx(a ^ (unsigned long long)vid[j]);
  return a;
}

// _h("chanmeta", n): every per-channel field derives from it
DEV unsigned long long yt_chanmeta_hash(unsigned long long base,
                                        unsigned long long n) {
  return yt_smx(yt_chain(base, "chanmeta") ^ n);
}

DEV int yt_video_count(unsigned long long base, unsigned long long n) {
  return (int)((yt_chanmeta_hash(base, n) >> 20) % 30ULL);
}

// channel_id_of (youtube/synth.py:82-91): 'UC' + 22 chars
DEV void yt_cid(unsigned long long seed_base, unsigned long long a_chan,
                long long n, unsigned char* out) {
  unsigned long long v = yt_smx(a_chan ^ (unsigned long long)n);
  out[0] = 'U';
  out[1] = 'C';
  for (int j = 0; j < 22; ++j) {
    out[2 + j] = (unsigned char)YT_ALPH[v % 62ULL];
    v = (v >> 5) | ((v & 31ULL) << 58);
    if (v < 62ULL) v = yt_smx(seed_base ^ v);
  }
}

DEV int yt_itoa(unsigned char* dst, long long v) {
  // non-negative itoa; returns digits written
  char tmp[20];
  int k = 0;
  do {
    tmp[k++] = (char)('0' + (v % 10));
    v /= 10;
  } while (v);
  for (int j = 0; j < k; ++j) dst[j] = (unsigned char)tmp[k - 1 - j];
  return k;
}

// grid for n elements at per_block elements per block; false = do not
// launch (n <= 0, or a grid past 0x7FFFFFFF)
static inline bool yt_grid(long long n, long long per_block,
                           unsigned int* grid) {
  if (n <= 0) return false;
  long long g = (n + per_block - 1) / per_block;
  if (g > 0x7FFFFFFFLL) return false;
  *grid = (unsigned int)g;
  return true;
}

}  // namespace crawl
