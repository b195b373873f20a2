// Per-channel fetch window: which rows of a K x P channel-grouped batch the
// crawl keeps (FetchChannelMessagesWithSampling, telegramutils.go:25-157;
// oracle: crawler_amd/ops/golden_window.py).
//
// A channel's rows are stored oldest first, so TDLib's newest-first walk
// is descending row index. Per channel:
//
//   for r = P-1 .. 0:
//     d = date[r]
//     if d > skip_above: continue        (skipped, the walk goes on)
//     if d < stop_below: break           (the walk ends, whatever is behind)
//     r is a candidate; stop once cap > 0 candidates are found
//   if sample_k > 0 and there are more than sample_k candidates:
//     keep the sample_k candidates with the smallest key(r)
//
//   key(r) = splitmix64(seed ^ (chat_id[r] * 0x9E3779B97F4A7C15 + msg_id[r]))
//
// in uint64 arithmetic. The key depends on the message's identity and the
// seed alone, so the sample does not change with the channel's place in a
// batch. Precondition: (chat_id, msg_id) is distinct within a channel;
// splitmix64 is a bijection, so the keys are distinct too and the k
// smallest are well defined.
//
// One wave per channel, blocks of 4 waves striding over the channels. The
// walk takes 64 rows per step, lane 0 the newest: a ballot of the stop
// predicate gives the first stopping lane, a ballot of the candidates in
// front of it their ranks (popcount of the lower lanes + the running
// count), and the rank is compared against cap. The sample's threshold,
// the sample_k-th smallest key, comes from a 64-round MSB-first radix
// select over the keys: from LDS (written by rank during the walk) when a
// channel has at most KEY_SLOTS candidates, recomputed from chat_id/msg_id
// otherwise. Every row's keep byte and every channel's kept count is
// written here; nothing relies on the buffers' previous contents.

#include "common.h"

namespace crawl {

constexpr int KEY_SLOTS = 1024;  // LDS keys per wave (8 KiB)

// the function of sample.hip / gpu.reservoir_sample_oracle
DEV unsigned long long splitmix64_w(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

DEV unsigned long long window_key(long seed, long chat, long msg) {
  return splitmix64_w((unsigned long long)seed ^
                      ((unsigned long long)chat * 0x9E3779B97F4A7C15ULL +
                       (unsigned long long)msg));
}

// The k-th smallest (k >= 1) of the keys get(j, key) yields over
// j = 0 .. iters-1 (get returns false where a lane has none). Bit by bit
// from the top: count the keys that share the chosen prefix and have a 0
// in this bit; the k-th lies among them, or behind them with a 1.
template <class F>
DEV unsigned long long kth_smallest(int iters, long k, F get) {
  unsigned long long prefix = 0;
  for (int b = 63; b >= 0; --b) {
    long zeros = 0;
    for (int j = 0; j < iters; ++j) {
      unsigned long long key = 0;
      bool have = get(j, key);
      zeros += __popcll(__ballot(have && ((key ^ prefix) >> b) == 0));
    }
    if (k > zeros) {
      k -= zeros;
      prefix |= 1ULL << b;
    }
  }
  return prefix;
}

__global__ void __launch_bounds__(256)
fetch_window_kernel(const int* __restrict__ date,
                    const long* __restrict__ chat_id,
                    const long* __restrict__ msg_id, int P, int n_channels,
                    long stop_below, long skip_above, long cap,
                    long sample_k, long seed, uint8_t* keep, int* kept) {
  __shared__ unsigned long long lds_keys[4][KEY_SLOTS];
  const int wave = wave_id();
  const int lane = lane_id();
  unsigned long long* keys = lds_keys[wave];
  const unsigned long long below = (1ULL << lane) - 1;
  const int ntiles = (P + WAVE - 1) / WAVE;

  for (int c = blockIdx.x * 4 + wave; c < n_channels; c += gridDim.x * 4) {
    const long base = (long)c * P;
    long running = 0;   // candidates so far (wave-uniform)
    bool done = false;  // the walk has ended (wave-uniform)
    int walked = 0;     // tiles the walk entered
    for (int t = 0; t < ntiles; ++t) {
      const int r = P - 1 - (t * WAVE + lane);
      const bool valid = r >= 0;
      bool cand = false;
      if (!done) {
        const long d = valid ? (long)date[base + r] : 0;
        const bool skip = d > skip_above;
        const unsigned long long stops =
            __ballot(valid && !skip && d < stop_below);
        const int first = stops ? __ffsll((long long)stops) - 1 : WAVE;
        cand = valid && !skip && lane < first;
        const long rank = running + __popcll(__ballot(cand) & below);
        if (cap > 0) cand = cand && rank < cap;
        if (sample_k > 0 && cand && rank < KEY_SLOTS)
          keys[rank] = window_key(seed, chat_id[base + r], msg_id[base + r]);
        running += __popcll(__ballot(cand));
        done = stops != 0 || (cap > 0 && running >= cap);
        walked = t + 1;
      }
      if (valid) keep[base + r] = cand ? 1 : 0;
    }

    if (sample_k > 0 && running > sample_k) {
      // the walk's LDS writes, before other lanes read them
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // a lane reads back the keep bytes it wrote itself (same r)
      auto from_rows = [&](int t, unsigned long long& key) {
        const int r = P - 1 - (t * WAVE + lane);
        if (r < 0 || !keep[base + r]) return false;
        key = window_key(seed, chat_id[base + r], msg_id[base + r]);
        return true;
      };
      unsigned long long kth;
      if (running <= KEY_SLOTS) {
        const int n = (int)running;
        kth = kth_smallest((n + WAVE - 1) / WAVE, sample_k,
                           [&](int j, unsigned long long& key) {
                             const int i = j * WAVE + lane;
                             if (i >= n) return false;
                             key = keys[i];
                             return true;
                           });
      } else {
        kth = kth_smallest(walked, sample_k, from_rows);
      }
      running = 0;
      for (int t = 0; t < walked; ++t) {
        unsigned long long key = 0;
        const bool in = from_rows(t, key) && key <= kth;
        const int r = P - 1 - (t * WAVE + lane);
        if (r >= 0) keep[base + r] = in ? 1 : 0;
        running += __popcll(__ballot(in));
      }
      // the next channel's walk overwrites the keys
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) kept[c] = (int)running;
  }
}

}  // namespace crawl

extern "C" {

int crawl_fetch_window(const void* date, const void* chat_id,
                       const void* msg_id, int posts_per_channel,
                       int n_channels, long stop_below, long skip_above,
                       long cap, long sample_k, long seed, void* keep,
                       void* kept, int grid, void* stream) {
  hipLaunchKernelGGL(crawl::fetch_window_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, (const int*)date,
                     (const long*)chat_id, (const long*)msg_id,
                     posts_per_channel, n_channels, stop_below, skip_above,
                     cap, sample_k, seed, (uint8_t*)keep, (int*)kept);
  return (int)hipGetLastError();
}

}  // extern "C"
