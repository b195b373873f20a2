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
//   crawl_yt_gen_meta_ids / crawl_yt_gen_fill_ids
//                          the yt_feedgen.hip meta/fill kernels driven by
//                          an id array instead of the i0 prefix walk
//   crawl_yt_chan_lens     channel-table string lengths
//
// One thread per output element, 256-thread blocks. Every entry point
// returns hipGetLastError() and launches nothing for a zero count.
#include "common.h"
#include "yt_hash.h"

namespace crawl {

#define YT_SEARCH_SLOTS 17
#define YT_UPLOAD_SLOTS 29
#define YT_CLAIM_EMPTY 0xFFFFFFFFFFFFFFFFULL

DEV unsigned long long yt_base(long long seed) {
  return (unsigned long long)seed ^ 0xC0FFEEULL;
}

// index of c in YT_ALPH, or -1
DEV int yt_alph_index(unsigned char c) {
  if (c >= 'a' && c <= 'z') return c - 'a';
  if (c >= 'A' && c <= 'Z') return 26 + (c - 'A');
  if (c >= '0' && c <= '9') return 52 + (c - '0');
  if (c == '-') return 62;
  if (c == '_') return 63;
  return -1;
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

DEV unsigned long long yt_vidmeta_hash(unsigned long long base,
                                       const unsigned char* vid) {
  unsigned long long a = yt_chain(base, "vidmeta");
  for (int j = 0; j < 11; ++j) a = yt_smx(a ^ (unsigned long long)vid[j]);
  return a;
}

DEV int yt_video_count(unsigned long long base, unsigned long long n) {
  unsigned long long hc = yt_smx(yt_chain(base, "chanmeta") ^ n);
  return (int)((hc >> 20) % 30ULL);
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

// ---------- id-driven meta / fill (yt_feedgen.hip semantics) ----------

__global__ void __launch_bounds__(256) yt_gen_meta_ids_kernel(
    long long seed, long long universe, long long base_date, long long n,
    const unsigned char* vid_pool /*[n,11]*/, long long* published,
    long long* views, int* likes, int* comments, int* duration_s,
    int* lang, long long* n_chan, int* topic, int* tnum, int* desc_len) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned char vid[11];
  for (int j = 0; j < 11; ++j) vid[j] = vid_pool[i * 11 + j];
  unsigned long long h = yt_vidmeta_hash(yt_base(seed), vid);
  n_chan[i] = (long long)(h % (unsigned long long)universe);
  int secs = (int)((h >> 8) % 7200ULL);
  duration_s[i] = secs ? secs : -1;
  published[i] = base_date + (long long)(h % 10000000ULL);
  views[i] = (long long)(h % 1000000ULL);
  likes[i] = (int)((h >> 12) % 50000ULL);
  comments[i] = (int)((h >> 22) % 5000ULL);
  lang[i] = (h % 4ULL) == 0 ? 1 : 0;  // LANGS: 0=en, 1=ru
  int tp = (int)(h % 1000ULL);
  int tn = (int)(h % 97ULL);
  topic[i] = tp;
  tnum[i] = tn;
  int dtp = tp >= 100 ? 3 : (tp >= 10 ? 2 : 1);
  int dtn = tn >= 10 ? 2 : 1;
  desc_len[i] = 18 + dtp + 29 + dtn + 45 + 24;
}

__global__ void __launch_bounds__(256) yt_gen_fill_ids_kernel(
    long long seed, long long universe, long long n,
    const unsigned char* vid_pool, const int* topic, const int* tnum,
    const long long* title_off, const long long* desc_off,
    unsigned char* pool) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned char vid[11];
  for (int j = 0; j < 11; ++j) vid[j] = vid_pool[i * 11 + j];
  for (int j = 0; j < 11; ++j) pool[i * 11 + j] = vid[j];
  const char* tp = "Synthetic video ";
  unsigned char* t = pool + title_off[i];
  for (int j = 0; j < 16; ++j) t[j] = (unsigned char)tp[j];
  for (int j = 0; j < 11; ++j) t[16 + j] = vid[j];
  unsigned char* d = pool + desc_off[i];
  const char* s1 = "Video about topic ";
  const char* s2 = ". More: https://example.com/t";
  const char* s3 = " and channel https://www.youtube.com/channel/";
  int c = 0;
  for (const char* p = s1; *p; ++p) d[c++] = (unsigned char)*p;
  c += yt_itoa(d + c, topic[i]);
  for (const char* p = s2; *p; ++p) d[c++] = (unsigned char)*p;
  c += yt_itoa(d + c, tnum[i]);
  for (const char* p = s3; *p; ++p) d[c++] = (unsigned char)*p;
  unsigned long long base = yt_base(seed);
  unsigned long long h = yt_vidmeta_hash(base, vid);
  yt_cid(base, yt_chain(base, "chan"),
         (long long)((h >> 13) % (unsigned long long)universe), d + c);
}

// channel-table string lengths: title "Synthetic YT Channel <n>", desc
// "Channel <n> description \xe2\x80\x94 see also UC friends", country
// "US" iff hc % 3 == 0
__global__ void __launch_bounds__(256) yt_chan_lens_kernel(
    long long seed, const long long* chan_ns, long long K,
    long long* title_len, long long* desc_len, long long* country_len) {
  long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= K) return;
  unsigned long long n = (unsigned long long)chan_ns[c];
  unsigned long long hc = yt_smx(yt_chain(yt_base(seed), "chanmeta") ^ n);
  int digs = u64_dec_len(n);
  title_len[c] = 21 + digs;
  desc_len[c] = 8 + digs + 36;
  country_len[c] = (hc % 3ULL == 0ULL) ? 2 : 0;
}

// 64-bit grid size for one thread per element; 0 = do not launch
static inline bool yt_grid(long long n, unsigned int* grid) {
  if (n <= 0) return false;
  long long g = (n + 255) / 256;
  if (g > 0x7FFFFFFFLL) return false;
  *grid = (unsigned int)g;
  return true;
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
      !crawl::yt_grid(S * YT_SEARCH_SLOTS, &grid))
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
  if (cap_log2 < 1 || cap_log2 > 40 || !crawl::yt_grid(n, &grid))
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
  if (cap_log2 < 1 || cap_log2 > 40 || !crawl::yt_grid(n, &grid))
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
  if (K > (1LL << 40) || !crawl::yt_grid(K * YT_UPLOAD_SLOTS, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_uploads_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, seed, (const long long*)chans,
                     K * YT_UPLOAD_SLOTS, limit, (unsigned char*)ids,
                     (int*)counts);
  return (int)hipGetLastError();
}

int crawl_yt_gen_meta_ids(long long seed, long long universe,
                          long long base_date, long long n,
                          const void* vid_pool, void* published,
                          void* views, void* likes, void* comments,
                          void* duration_s, void* lang, void* n_chan,
                          void* topic, void* tnum, void* desc_len,
                          void* stream) {
  unsigned int grid;
  if (n <= 0) return (int)hipGetLastError();
  if (universe <= 0 || !crawl::yt_grid(n, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_gen_meta_ids_kernel, dim3(grid), dim3(256),
                     0, (hipStream_t)stream, seed, universe, base_date, n,
                     (const unsigned char*)vid_pool, (long long*)published,
                     (long long*)views, (int*)likes, (int*)comments,
                     (int*)duration_s, (int*)lang, (long long*)n_chan,
                     (int*)topic, (int*)tnum, (int*)desc_len);
  return (int)hipGetLastError();
}

int crawl_yt_gen_fill_ids(long long seed, long long universe, long long n,
                          const void* vid_pool, const void* topic,
                          const void* tnum, const void* title_off,
                          const void* desc_off, void* pool, void* stream) {
  unsigned int grid;
  if (n <= 0) return (int)hipGetLastError();
  if (universe <= 0 || !crawl::yt_grid(n, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_gen_fill_ids_kernel, dim3(grid), dim3(256),
                     0, (hipStream_t)stream, seed, universe, n,
                     (const unsigned char*)vid_pool, (const int*)topic,
                     (const int*)tnum, (const long long*)title_off,
                     (const long long*)desc_off, (unsigned char*)pool);
  return (int)hipGetLastError();
}

int crawl_yt_chan_lens(long long seed, const void* chan_ns, long long K,
                       void* title_len, void* desc_len, void* country_len,
                       void* stream) {
  unsigned int grid;
  if (K <= 0) return (int)hipGetLastError();
  if (!crawl::yt_grid(K, &grid)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_chan_lens_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, seed, (const long long*)chan_ns,
                     K, (long long*)title_len, (long long*)desc_len,
                     (long long*)country_len);
  return (int)hipGetLastError();
}

}  // extern "C"
