// Device-side YouTube synthetic-index generation — the YouTube half of
// the C++/HIP synthetic-API engine (the Telegram half is
// feedgen.hip), and the only home of the generator kernels. Generates
// the packed YouTubeBatch pools directly in HBM, byte-identical to the
// numpy reference builder (youtube/batch.py build_corpus_fast, itself
// pinned to the per-video python path by tests).
//
// Everything is driven by an id array (uint8[n,11]); torch cumsums and
// unique run between the phases:
//   crawl_yt_gen_ids       the ids of rows i0 .. i0+n-1 of the prefix
//                          walk (search hits and uploads bring their own)
//   crawl_yt_gen_meta      per-video numeric fields, channel index,
//                          description length
//   crawl_yt_gen_fill      vid/title/desc pool bytes (incl. the linked
//                          channel id)
//   crawl_yt_chan_lens     channel-table string lengths
//   crawl_yt_gen_channels  channel-table fields and pool bytes
//
// One thread per output element, 256-thread blocks. Every entry point
// launches nothing for a count <= 0 and returns hipGetLastError(); an
// impossible argument returns hipErrorInvalidValue.
#include "common.h"
#include "yt_hash.h"

namespace crawl {

// row i of the prefix walk (build_corpus): the prefix is the low five
// base-26 digits of i, so it wraps at 26^5; k = i % 7
__global__ void __launch_bounds__(256) yt_gen_ids_kernel(
    long long seed, long long i0, long long n,
    unsigned char* vid_pool /*[n,11]*/) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  long long i = i0 + t;
  long long v = i;
  unsigned char pc[5];
  for (int j = 4; j >= 0; --j) {
    pc[j] = (unsigned char)('a' + (v % 26));
    v /= 26;
  }
  unsigned char vid[11];
  yt_video_id(yt_base(seed), pc, (unsigned long long)(i % 7), vid);
  for (int j = 0; j < 11; ++j) vid_pool[t * 11 + j] = vid[j];
}

__global__ void __launch_bounds__(256) yt_gen_meta_kernel(
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
  // "Video about topic " (18) + d(tp) + ". More: https://example.com/t"
  // (29) + d(tn) + " and channel https://www.youtube.com/channel/" (45)
  // + 24-char channel id
  desc_len[i] = 18 + dtp + 29 + dtn + 45 + 24;
}

__global__ void __launch_bounds__(256) yt_gen_fill_kernel(
    long long seed, long long universe, long long n,
    const unsigned char* vid_pool, const int* topic, const int* tnum,
    const long long* title_off, const long long* desc_off,
    unsigned char* pool) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned char vid[11];
  for (int j = 0; j < 11; ++j) vid[j] = vid_pool[i * 11 + j];
  // vid region: pool[0 .. n*11) with stride 11 (host sets vid_off)
  for (int j = 0; j < 11; ++j) pool[i * 11 + j] = vid[j];
  // title: "Synthetic video " + vid (27 bytes)
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
  // link channel id: (h >> 13) % universe
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
  unsigned long long hc = yt_chanmeta_hash(yt_base(seed), n);
  int digs = u64_dec_len(n);
  title_len[c] = 21 + digs;
  desc_len[c] = 8 + digs + 36;
  country_len[c] = (hc % 3ULL == 0ULL) ? 2 : 0;
}

__global__ void __launch_bounds__(256) yt_gen_channels_kernel(
    long long seed, long long base_date, const long long* chan_ns,
    long long K, const long long* id_off, const long long* title_off,
    const long long* desc_off, const long long* country_off,
    long long* subs, int* videos, long long* ch_views,
    long long* ch_published, unsigned char* pool) {
  long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= K) return;
  long long n = chan_ns[c];
  unsigned long long base = yt_base(seed);
  unsigned long long hc = yt_chanmeta_hash(base, (unsigned long long)n);
  subs[c] = (long long)(hc % 1000000ULL);
  videos[c] = yt_video_count(base, (unsigned long long)n);
  ch_views[c] = (long long)((hc >> 25) % 50000000ULL);
  ch_published[c] = base_date - (long long)(hc % 100000000ULL);
  yt_cid(base, yt_chain(base, "chan"), n, pool + id_off[c]);
  // title: "Synthetic YT Channel " + n
  const char* t1 = "Synthetic YT Channel ";
  unsigned char* t = pool + title_off[c];
  int k = 0;
  for (const char* p = t1; *p; ++p) t[k++] = (unsigned char)*p;
  yt_itoa(t + k, n);
  // desc: "Channel " + n + " description \xe2\x80\x94 see also UC friends"
  const char* d1 = "Channel ";
  const char* d2 = " description \xe2\x80\x94 see also UC friends";
  unsigned char* d = pool + desc_off[c];
  k = 0;
  for (const char* p = d1; *p; ++p) d[k++] = (unsigned char)*p;
  k += yt_itoa(d + k, n);
  for (const char* p = d2; *p; ++p) d[k++] = (unsigned char)*p;
  // country: "US" when hc % 3 == 0 (yt_chan_lens_kernel sized it)
  if (hc % 3ULL == 0ULL) {
    unsigned char* u = pool + country_off[c];
    u[0] = 'U';
    u[1] = 'S';
  }
}

}  // namespace crawl

extern "C" {

int crawl_yt_gen_ids(long long seed, long long i0, long long n,
                     void* vid_pool, void* stream) {
  unsigned int grid;
  if (n <= 0) return (int)hipGetLastError();
  if (i0 < 0 || i0 > 0x7FFFFFFFFFFFFFFFLL - n ||
      !crawl::yt_grid(n, 256, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_gen_ids_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, seed, i0, n,
                     (unsigned char*)vid_pool);
  return (int)hipGetLastError();
}

int crawl_yt_gen_meta(long long seed, long long universe,
                      long long base_date, long long n,
                      const void* vid_pool, void* published, void* views,
                      void* likes, void* comments, void* duration_s,
                      void* lang, void* n_chan, void* topic, void* tnum,
                      void* desc_len, void* stream) {
  unsigned int grid;
  if (n <= 0) return (int)hipGetLastError();
  if (universe <= 0 || !crawl::yt_grid(n, 256, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_gen_meta_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, seed, universe, base_date, n,
                     (const unsigned char*)vid_pool, (long long*)published,
                     (long long*)views, (int*)likes, (int*)comments,
                     (int*)duration_s, (int*)lang, (long long*)n_chan,
                     (int*)topic, (int*)tnum, (int*)desc_len);
  return (int)hipGetLastError();
}

int crawl_yt_gen_fill(long long seed, long long universe, long long n,
                      const void* vid_pool, const void* topic,
                      const void* tnum, const void* title_off,
                      const void* desc_off, void* pool, void* stream) {
  unsigned int grid;
  if (n <= 0) return (int)hipGetLastError();
  if (universe <= 0 || !crawl::yt_grid(n, 256, &grid))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_gen_fill_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, seed, universe, n,
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
  if (!crawl::yt_grid(K, 256, &grid)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_chan_lens_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, seed, (const long long*)chan_ns,
                     K, (long long*)title_len, (long long*)desc_len,
                     (long long*)country_len);
  return (int)hipGetLastError();
}

int crawl_yt_gen_channels(long long seed, long long base_date,
                          const void* chan_ns, long long K,
                          const void* id_off, const void* title_off,
                          const void* desc_off, const void* country_off,
                          void* subs, void* videos, void* ch_views,
                          void* ch_published, void* pool, void* stream) {
  unsigned int grid;
  if (K <= 0) return (int)hipGetLastError();
  if (!crawl::yt_grid(K, 256, &grid)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crawl::yt_gen_channels_kernel, dim3(grid), dim3(256),
                     0, (hipStream_t)stream, seed, base_date,
                     (const long long*)chan_ns, K,
                     (const long long*)id_off,
                     (const long long*)title_off,
                     (const long long*)desc_off,
                     (const long long*)country_off, (long long*)subs,
                     (int*)videos, (long long*)ch_views,
                     (long long*)ch_published, (unsigned char*)pool);
  return (int)hipGetLastError();
}

}  // extern "C"
