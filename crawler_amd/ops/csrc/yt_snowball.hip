// Device-side YouTube snowball discovery — the GPU half of
// GetSnowballVideos' channel-id extraction (youtube/client.py
// extract_channel_ids_from_text) and of channel_index_of:
//
//   crawl_yt_scan_count / crawl_yt_scan_write
//                          leftmost non-overlapping matches of
//                          UC[0-9A-Za-z_-]{22} in packed texts
//                          (measure / write, one shared routine)
//   crawl_yt_cid_table_build
//                          channel id -> channel index reverse map over
//                          the whole universe (open addressing)
//   crawl_yt_cid_lookup    24 id bytes at a pool offset -> index or -1
//
// The scan runs one 64-lane wave per text, four waves per block; the
// reverse map one thread per element, 256-thread blocks. Every entry
// point returns hipGetLastError() and launches nothing for a zero count.
#include "common.h"
#include "yt_hash.h"

namespace crawl {

#define YT_CID_LEN 24
#define YT_CID_EMPTY 0xFFFFFFFFFFFFFFFFULL
#define YT_SCAN_WAVES 4

// [0-9A-Za-z_-]; a byte >= 0x80 is never a class byte
DEV bool yt_cid_class(unsigned char c) {
  return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') ||
         (c >= 'a' && c <= 'z') || c == '_' || c == '-';
}

// (lo, hi) is a 128-bit window, hi the upper word; returns the upper
// word of the window shifted left by s (0 < s < 64)
DEV unsigned long long yt_shl_hi(unsigned long long lo,
                                 unsigned long long hi, int s) {
  return (hi << s) | (lo >> (64 - s));
}

// Scan one text with one wave. Each lane reads ONE byte per 64-byte
// chunk; three ballots give the chunk's class / 'U' / 'C' masks, and
// the previous chunk's masks are carried so that a match may straddle
// the boundary. A match is found at its LAST byte q: the 22 bytes
// q-21..q are class bytes, byte q-22 is 'C' and byte q-23 is 'U'. The
// class-run mask comes from shift-and-AND doubling (runs of 2, 4, 8, 16,
// then 16 + 6 = 22). Lanes past the text's end contribute zero bits, so
// no byte outside [text, text + len) is read or can complete a match.
// Leftmost non-overlap is the wave-uniform walk over the end mask with
// next_free carried across chunks. W = false counts, W = true also
// writes each match's absolute pool offset. Returns the match count.
template <bool W>
DEV int yt_scan_text(const unsigned char* pool, long long off, int len,
                     long long* out) {
  int lane = lane_id();
  unsigned long long k_lo = 0, u_lo = 0, c_lo = 0;
  long long next_free = 0;  // text-relative
  int count = 0;
  for (int base = 0; base < len; base += WAVE) {
    int p = base + lane;
    unsigned char b = p < len ? pool[off + p] : (unsigned char)0;
    unsigned long long k_hi = __ballot(yt_cid_class(b));
    unsigned long long u_hi = __ballot(b == 'U');
    unsigned long long c_hi = __ballot(b == 'C');
    // runs of class bytes ending at each position. The zeros shifted
    // into the low word spoil only its bits < 15 (1 + 2 + 4 + 8), and
    // the upper word's results read no low-word bit below 41.
    unsigned long long a1_lo = k_lo & (k_lo << 1);
    unsigned long long a1_hi = k_hi & yt_shl_hi(k_lo, k_hi, 1);
    unsigned long long a2_lo = a1_lo & (a1_lo << 2);
    unsigned long long a2_hi = a1_hi & yt_shl_hi(a1_lo, a1_hi, 2);
    unsigned long long a4_lo = a2_lo & (a2_lo << 4);
    unsigned long long a4_hi = a2_hi & yt_shl_hi(a2_lo, a2_hi, 4);
    unsigned long long a8_lo = a4_lo & (a4_lo << 8);
    unsigned long long a8_hi = a4_hi & yt_shl_hi(a4_lo, a4_hi, 8);
    unsigned long long run22 = a8_hi & yt_shl_hi(a8_lo, a8_hi, 6);
    unsigned long long ends = run22 & yt_shl_hi(c_lo, c_hi, 22) &
                              yt_shl_hi(u_lo, u_hi, 23);
    while (ends) {
      int bit = __builtin_ctzll(ends);
      ends &= ends - 1ULL;
      long long start = (long long)base + bit - (YT_CID_LEN - 1);
      if (start >= next_free) {
        if (W && lane == 0) out[count] = off + start;
        ++count;
        next_free = start + YT_CID_LEN;
      }
    }
    k_lo = k_hi;
    u_lo = u_hi;
    c_lo = c_hi;
  }
  return count;
}

template <bool W>
__global__ void __launch_bounds__(64 * YT_SCAN_WAVES) yt_scan_kernel(
    const unsigned char* pool, const long long* text_off,
    const int* text_len, long long n, const long long* out_base,
    int* counts, long long* hit_off) {
  long long t = (long long)blockIdx.x * YT_SCAN_WAVES + wave_id();
  if (t >= n) return;
  int len = text_len[t];
  if (len < 0) len = 0;
  long long* out = W ? hit_off + out_base[t] : nullptr;
  int c = yt_scan_text<W>(pool, text_off[t], len, out);
  if (!W && lane_id() == 0) counts[t] = c;
}

// ---------- channel id -> channel index ----------
// Open addressing over table[cap] (cap = 1 << cap_log2) of channel
// indices; the slot comes from a hash of the 22 id characters, linear
// probing with wrap-around, every probe loop bounded by cap. No strings
// are stored: a slot's id is regenerated from its index.

DEV unsigned long long yt_cid_hash22(const unsigned char* id24) {
  unsigned long long h = 1469598103934665603ULL;
  for (int j = 2; j < YT_CID_LEN; ++j) {
    h ^= id24[j];
    h *= 1099511628211ULL;
  }
  return yt_smx(h);
}

DEV bool yt_cid_equal(const unsigned char* a, const unsigned char* b) {
  bool eq = true;
  for (int j = 0; j < YT_CID_LEN; ++j) eq = eq && a[j] == b[j];
  return eq;
}

__global__ void __launch_bounds__(256) yt_cid_table_build_kernel(
    long long seed, long long universe, unsigned long long* table,
    unsigned long long cap, unsigned int* err) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= universe) return;
  unsigned long long base = yt_base(seed);
  unsigned long long a_chan = yt_chain(base, "chan");
  unsigned char id[YT_CID_LEN];
  yt_cid(base, a_chan, i, id);
  unsigned long long cap_mask = cap - 1ULL;
  unsigned long long slot = yt_cid_hash22(id) & cap_mask;
  for (unsigned long long p = 0; p < cap; ++p) {
    unsigned long long prev =
        atomicCAS(&table[slot], YT_CID_EMPTY, (unsigned long long)i);
    if (prev == YT_CID_EMPTY) return;
    // occupied: the same id (a duplicate) keeps the smaller index.
    // A slot's value only ever moves between indices of ONE id, so the
    // comparison below does not depend on when prev was read.
    unsigned char other[YT_CID_LEN];
    yt_cid(base, a_chan, (long long)prev, other);
    if (yt_cid_equal(id, other)) {
      atomicMin(&table[slot], (unsigned long long)i);
      return;
    }
    slot = (slot + 1ULL) & cap_mask;
  }
  atomicOr(err, 1u);  // table full: wrapped without a home
}

__global__ void __launch_bounds__(256) yt_cid_lookup_kernel(
    long long seed, const unsigned char* pool, const long long* hit_off,
    long long m, const unsigned long long* table, unsigned long long cap,
    long long* out_n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  unsigned long long base = yt_base(seed);
  unsigned long long a_chan = yt_chain(base, "chan");
  unsigned char id[YT_CID_LEN];
  const unsigned char* src = pool + hit_off[i];
  for (int j = 0; j < YT_CID_LEN; ++j) id[j] = src[j];
  unsigned long long cap_mask = cap - 1ULL;
  unsigned long long slot = yt_cid_hash22(id) & cap_mask;
  long long found = -1;
  for (unsigned long long p = 0; p < cap; ++p) {
    unsigned long long v = table[slot];
    if (v == YT_CID_EMPTY) break;
    unsigned char other[YT_CID_LEN];
    yt_cid(base, a_chan, (long long)v, other);
    if (yt_cid_equal(id, other)) {
      found = (long long)v;
      break;
    }
    slot = (slot + 1ULL) & cap_mask;
  }
  out_n[i] = found;
}

}  // namespace crawl

extern "C" {

// pass 1: counts[t] = matches in text t
int crawl_yt_scan_count(const void* pool, const void* text_off,
                        const void* text_len, long long n, void* counts,
                        void* stream) {
  unsigned int grid;
  if (n <= 0) return (int)hipGetLastError();
  if (!crawl::yt_grid(n, YT_SCAN_WAVES, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_scan_kernel<false>, dim3(grid),
                     dim3(64 * YT_SCAN_WAVES), 0, (hipStream_t)stream,
                     (const unsigned char*)pool, (const long long*)text_off,
                     (const int*)text_len, n, (const long long*)nullptr,
                     (int*)counts, (long long*)nullptr);
  return (int)hipGetLastError();
}

// pass 2: out_base[t] = exclusive cumsum of counts; hit_off receives each
// match's absolute pool offset, in text order then match order
int crawl_yt_scan_write(const void* pool, const void* text_off,
                        const void* text_len, long long n,
                        const void* out_base, void* hit_off,
                        void* stream) {
  unsigned int grid;
  if (n <= 0) return (int)hipGetLastError();
  if (!crawl::yt_grid(n, YT_SCAN_WAVES, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_scan_kernel<true>, dim3(grid),
                     dim3(64 * YT_SCAN_WAVES), 0, (hipStream_t)stream,
                     (const unsigned char*)pool, (const long long*)text_off,
                     (const int*)text_len, n, (const long long*)out_base,
                     (int*)nullptr, (long long*)hit_off);
  return (int)hipGetLastError();
}

// table[1 << cap_log2] must be filled with all-ones (empty) by the
// caller; err bit 0 = table full
int crawl_yt_cid_table_build(long long seed, long long universe,
                             void* table, int cap_log2, void* err,
                             void* stream) {
  unsigned int grid;
  if (universe <= 0) return (int)hipGetLastError();
  if (cap_log2 < 1 || cap_log2 > 40 ||
      !crawl::yt_grid(universe, 256, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_cid_table_build_kernel, dim3(grid),
                     dim3(256), 0, (hipStream_t)stream, seed, universe,
                     (unsigned long long*)table, 1ULL << cap_log2,
                     (unsigned int*)err);
  return (int)hipGetLastError();
}

// out_n[i] = channel index of the 24 bytes at pool + hit_off[i], or -1
int crawl_yt_cid_lookup(long long seed, const void* pool,
                        const void* hit_off, long long m,
                        const void* table, int cap_log2, void* out_n,
                        void* stream) {
  unsigned int grid;
  if (m <= 0) return (int)hipGetLastError();
  if (cap_log2 < 1 || cap_log2 > 40 || !crawl::yt_grid(m, 256, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_cid_lookup_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, seed,
                     (const unsigned char*)pool, (const long long*)hit_off,
                     m, (const unsigned long long*)table, 1ULL << cap_log2,
                     (long long*)out_n);
  return (int)hipGetLastError();
}

}  // extern "C"
