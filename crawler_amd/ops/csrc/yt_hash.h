// splitmix64 hash helpers of the synthetic YouTube index
// (youtube/synth.py SyntheticYouTubeIndex._h and friends), shared by the
// device generators (yt_feedgen.hip) and the sampling kernels
// (yt_sample.hip).
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

}  // namespace crawl
