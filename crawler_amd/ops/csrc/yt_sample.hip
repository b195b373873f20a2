// Device-side YouTube sampling — the GPU half of GetRandomVideos and of
// channel sampling (youtube/client.py, youtube/synth.py):
//
//   crawl_yt_search        search_prefix + the validity rule, 17 slots
//                          per prefix
//   crawl_yt_first_claim   deterministic first-occurrence marking over
//                          64-bit keys (the client's `seen` set and its
//                          channel cache)
//   crawl_yt_claim_insert  pass 1 alone (re-insert on table growth)
//   crawl_yt_uploads       channel_uploads, 29 slots per channel
//
// The ids found here become batches through the generator kernels of
// yt_feedgen.hip; the index's hash helpers are in yt_hash.h.
//
// One thread per output element, 256-thread blocks. Every entry point
// returns hipGetLastError() and launches nothing for a zero count.
#include "common.h"
#include "yt_hash.h"

namespace crawl {

#define YT_SEARCH_SLOTS 17
#define YT_UPLOAD_SLOTS 29
#define YT_CLAIM_EMPTY 0xFFFFFFFFFFFFFFFFULL

// index of c in YT_ALPH, or -1
DEV int yt_alph_index(unsigned char c) {
  if (c >= 'a' && c <= 'z') return c - 'a';
  if (c >= 'A' && c <= 'Z') return 26 + (c - 'A');
  if (c >= '0' && c <= '9') return 52 + (c - '0');
  if (c == '-') return 62;
  if (c == '_') return 63;
  return -1;
}

// ---------- search ----------

__global__ void __launch_bounds__(256) yt_search_kernel(
    long long seed, long long universe, const unsigned char* prefixes,
    long long n_slots, unsigned char* ids /*[S,17,11]*/,
    unsigned char* flags /*[S,17]*/, unsigned long long* keys,
    long long* chan, int* vcount) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots) return;
  long long s = t / YT_SEARCH_SLOTS;
  int j = (int)(t % YT_SEARCH_SLOTS);
  unsigned long long base = yt_base(seed);
  unsigned char pc[5];
  for (int i = 0; i < 5; ++i) pc[i] = prefixes[s * 5 + i];
  unsigned long long h = yt_chain(base, "search");
  for (int i = 0; i < 5; ++i) h = yt_smx(h ^ (unsigned long long)pc[i]);
  int n_valid = (int)(h % 6ULL);
  int n_noise = 3 + (int)((h >> 8) % 10ULL);
  unsigned char vid[11];
  bool present = j < n_valid + n_noise;
  if (j < n_valid) {
    yt_video_id(base, pc, (unsigned long long)j, vid);
  } else if (present) {
    // noise_id(h + s): the salt wraps mod 2^64 like _h's mask
    unsigned long long salt = h + (unsigned long long)(j - n_valid);
    unsigned long long hn = yt_smx(yt_chain(base, "noise") ^ salt);
    for (int i = 0; i < 11; ++i)
      vid[i] = (unsigned char)YT_ALPH[(hn >> (6 * i)) % 64ULL];
  } else {
    for (int i = 0; i < 11; ++i) vid[i] = 0;
  }
  // validity rule on the produced bytes: starts with the prefix and
  // id[5] == '-' (the length is 11 by construction)
  bool valid = present && vid[5] == '-';
  for (int i = 0; i < 5; ++i) valid = valid && vid[i] == pc[i];
  unsigned long long key = 0;
  if (valid) {
    // injective key: base-26 prefix (< 2^24) << 30 | five 6-bit tail
    // indices; < 2^54, so never the table's all-ones empty sentinel.
    // A prefix char outside a-z cannot be packed: the slot is dropped.
    unsigned long long p26 = 0;
    for (int i = 0; i < 5; ++i) {
      if (pc[i] < 'a' || pc[i] > 'z') valid = false;
      p26 = p26 * 26ULL + (unsigned long long)(pc[i] - 'a');
    }
    key = p26 << 30;
    for (int i = 0; i < 5; ++i) {
      int a = yt_alph_index(vid[6 + i]);
      if (a < 0) valid = false;
      key |= (unsigned long long)(a & 63) << (6 * i);
    }
  }
  for (int i = 0; i < 11; ++i) ids[t * 11 + i] = vid[i];
  flags[t] = (unsigned char)((present ? 1 : 0) | (valid ? 2 : 0));
  long long nc = -1;
  int vc = 0;
  if (valid) {
    nc = (long long)(yt_vidmeta_hash(base, vid) %
                     (unsigned long long)universe);
    vc = yt_video_count(base, (unsigned long long)nc);
  } else {
    key = 0;
  }
  keys[t] = key;
  chan[t] = nc;
  vcount[t] = vc;
}

// ---------- first-claim table ----------
// Open addressing over keys[cap] / min_idx[cap], cap = 1 << cap_log2,
// linear probing with wrap-around. Every probe loop is bounded by cap.

DEV unsigned long long yt_claim_slot0(unsigned long long key,
                                      unsigned long long cap_mask) {
  return yt_smx(key) & cap_mask;
}

// pass 1: insert the key, atomicMin the element's global index
__global__ void __launch_bounds__(256) yt_claim_insert_kernel(
    const unsigned long long* keys_in, const unsigned char* mask,
    const long long* idx_in, long long n, long long base_idx,
    unsigned long long* tab_keys, unsigned long long* tab_min,
    unsigned long long cap, unsigned int* err) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (mask && !mask[i]) return;
  unsigned long long key = keys_in[i];
  unsigned long long idx =
      (unsigned long long)(idx_in ? idx_in[i] : base_idx + i);
  if (key == YT_CLAIM_EMPTY) {
    atomicOr(err, 2u);
    return;
  }
  unsigned long long cap_mask = cap - 1ULL;
  unsigned long long slot = yt_claim_slot0(key, cap_mask);
  for (unsigned long long p = 0; p < cap; ++p) {
    unsigned long long prev = atomicCAS(&tab_keys[slot], YT_CLAIM_EMPTY, key);
    if (prev == YT_CLAIM_EMPTY || prev == key) {
      atomicMin(&tab_min[slot], idx);
      return;
    }
    slot = (slot + 1ULL) & cap_mask;
  }
  atomicOr(err, 1u);  // table full: wrapped without a home
}

// pass 2 (separate launch: ordered after every insert): first iff the
// key's min index is this element's own
__global__ void __launch_bounds__(256) yt_claim_resolve_kernel(
    const unsigned long long* keys_in, const unsigned char* mask,
    long long n, long long base_idx, const unsigned long long* tab_keys,
    const unsigned long long* tab_min, unsigned long long cap,
    unsigned char* first, unsigned int* err) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned char f = 0;
  if (!mask || mask[i]) {
    unsigned long long key = keys_in[i];
    unsigned long long idx = (unsigned long long)(base_idx + i);
    unsigned long long cap_mask = cap - 1ULL;
    unsigned long long slot = yt_claim_slot0(key, cap_mask);
    bool found = false;
    for (unsigned long long p = 0; p < cap; ++p) {
      unsigned long long k = tab_keys[slot];
      if (k == key) {
        f = tab_min[slot] == idx ? 1 : 0;
        found = true;
        break;
      }
      if (k == YT_CLAIM_EMPTY) break;
      slot = (slot + 1ULL) & cap_mask;
    }
    if (!found) atomicOr(err, 1u);
  }
  first[i] = f;
}

// ---------- channel uploads ----------

__global__ void __launch_bounds__(256) yt_uploads_kernel(
    long long seed, const long long* chans, long long n_slots, int limit,
    unsigned char* ids /*[K,29,11]*/, int* counts /*[K]*/) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots) return;
  long long c = t / YT_UPLOAD_SLOTS;
  int k = (int)(t % YT_UPLOAD_SLOTS);
  unsigned long long base = yt_base(seed);
  unsigned long long n = (unsigned long long)chans[c];
  int cnt = yt_video_count(base, n);
  if (cnt > limit) cnt = limit;
  if (cnt < 0) cnt = 0;
  if (k == 0) counts[c] = cnt;
  unsigned char vid[11];
  if (k < cnt) {
    unsigned long long h = yt_smx(yt_chain(base, "upload") ^ n);
    h = yt_smx(h ^ (unsigned long long)k);
    unsigned char pc[5];
    for (int i = 0; i < 5; ++i)
      pc[i] = (unsigned char)('a' + (h >> (5 * i)) % 26ULL);
    yt_video_id(base, pc, h % 7ULL, vid);
  } else {
    for (int i = 0; i < 11; ++i) vid[i] = 0;
  }
  for (int i = 0; i < 11; ++i) ids[t * 11 + i] = vid[i];
}

}  // namespace crawl

extern "C" {

int crawl_yt_search(long long seed, long long universe,
                    const void* prefixes, long long S, void* ids,
                    void* flags, void* keys, void* chan, void* vcount,
                    void* stream) {
  unsigned int grid;
  if (S <= 0) return (int)hipGetLastError();
  if (S > (1LL << 40) || universe <= 0 ||
      !crawl::yt_grid(S * YT_SEARCH_SLOTS, 256, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_search_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, seed, universe,
                     (const unsigned char*)prefixes, S * YT_SEARCH_SLOTS,
                     (unsigned char*)ids, (unsigned char*)flags,
                     (unsigned long long*)keys, (long long*)chan,
                     (int*)vcount);
  return (int)hipGetLastError();
}

int crawl_yt_claim_insert(const void* keys_in, const void* mask,
                          const void* idx_in, long long n,
                          long long base_idx, void* tab_keys,
                          void* tab_min, int cap_log2, void* err,
                          void* stream) {
  unsigned int grid;
  if (n <= 0) return (int)hipGetLastError();
  if (cap_log2 < 1 || cap_log2 > 40 || !crawl::yt_grid(n, 256, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_claim_insert_kernel, dim3(grid), dim3(256),
                     0, (hipStream_t)stream,
                     (const unsigned long long*)keys_in,
                     (const unsigned char*)mask, (const long long*)idx_in,
                     n, base_idx, (unsigned long long*)tab_keys,
                     (unsigned long long*)tab_min, 1ULL << cap_log2,
                     (unsigned int*)err);
  return (int)hipGetLastError();
}

int crawl_yt_first_claim(const void* keys_in, const void* mask,
                         long long n, long long base_idx, void* tab_keys,
                         void* tab_min, int cap_log2, void* first,
                         void* err, void* stream) {
  unsigned int grid;
  if (n <= 0) return (int)hipGetLastError();
  if (cap_log2 < 1 || cap_log2 > 40 || !crawl::yt_grid(n, 256, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_claim_insert_kernel, dim3(grid), dim3(256),
                     0, (hipStream_t)stream,
                     (const unsigned long long*)keys_in,
                     (const unsigned char*)mask, (const long long*)nullptr,
                     n, base_idx, (unsigned long long*)tab_keys,
                     (unsigned long long*)tab_min, 1ULL << cap_log2,
                     (unsigned int*)err);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(crawl::yt_claim_resolve_kernel, dim3(grid), dim3(256),
                     0, (hipStream_t)stream,
                     (const unsigned long long*)keys_in,
                     (const unsigned char*)mask, n, base_idx,
                     (const unsigned long long*)tab_keys,
                     (const unsigned long long*)tab_min, 1ULL << cap_log2,
                     (unsigned char*)first, (unsigned int*)err);
  return (int)hipGetLastError();
}

int crawl_yt_uploads(long long seed, const void* chans, long long K,
                     int limit, void* ids, void* counts, void* stream) {
  unsigned int grid;
  if (K <= 0) return (int)hipGetLastError();
  if (K > (1LL << 40) ||
      !crawl::yt_grid(K * YT_UPLOAD_SLOTS, 256, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_uploads_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, seed, (const long long*)chans,
                     K * YT_UPLOAD_SLOTS, limit, (unsigned char*)ids,
                     (int*)counts);
  return (int)hipGetLastError();
}

}  // extern "C"
