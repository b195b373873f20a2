// Channel activity gate and kept-row compaction for a K x P
// channel-grouped batch that went through the fetch window
// (fetch_window.hip). Oracle: crawler_amd/ops/golden_gate.py.
//
// Gate (isChannelActiveWithinPeriod, runner.go:628-643): a channel whose
// newest message is not newer than the recency cutoff is a deadend; it
// writes no post and none of its links is followed. Per channel c:
//
//   kept[c] > 0:  latest = max(date[r] for the rows with keep[r] != 0)
//                 (the newest of the fetched messages)
//   kept[c] == 0: latest = date of the row with the greatest msg_id
//                 (GetChatHistory(limit=1): the chat's newest message;
//                 of equal msg_ids the lowest row)
//   active = latest > recency       (a tie is inactive)
//   inactive: every keep byte of the channel is cleared, kept[c] = 0
//
// Nothing here assumes that dates are monotone or that the newest
// message sits in row P-1.
//
// Compaction: channel c writes the global indices of its kept rows,
// ascending, to rows[kept_offset[c] ..) and c to the same slots of
// row_channel. kept_offset holds K + 1 entries, the exclusive prefix sum
// of kept with the total behind it, so a channel knows where its range
// ends: a keep mask with more rows than kept[c] loses the surplus
// instead of writing past its range.
//
// Both kernels: one wave per channel, blocks of 4 waves striding over
// the channels, 64 rows per step. Rows past P in the last tile take part
// in nothing. Every element of active and latest is written.

#include <limits.h>

#include "common.h"

namespace crawl {

__global__ void __launch_bounds__(256)
channel_gate_kernel(const int* __restrict__ date,
                    const long* __restrict__ msg_id, int P, int n_channels,
                    long recency, uint8_t* keep, int* kept, uint8_t* active,
                    int* latest) {
  const int wave = wave_id();
  const int lane = lane_id();
  const int ntiles = (P + WAVE - 1) / WAVE;

  for (int c = blockIdx.x * 4 + wave; c < n_channels; c += gridDim.x * 4) {
    const long base = (long)c * P;
    const bool fetched = kept[c] > 0;  // wave-uniform
    int newest;
    if (fetched) {
      int best = INT_MIN;
      for (int t = 0; t < ntiles; ++t) {
        const int r = t * WAVE + lane;
        if (r < P && keep[base + r]) {
          const int d = date[base + r];
          best = d > best ? d : best;
        }
      }
      for (int s = WAVE / 2; s > 0; s >>= 1) {
        const int o = __shfl_xor(best, s);
        best = o > best ? o : best;
      }
      newest = best;
    } else {
      long long best_id = LLONG_MIN;
      int best_row = INT_MAX;
      for (int t = 0; t < ntiles; ++t) {
        const int r = t * WAVE + lane;
        if (r < P) {
          const long long m = msg_id[base + r];
          // rows ascend within a lane, so an equal id keeps the lower
          if (best_row == INT_MAX || m > best_id) {
            best_id = m;
            best_row = r;
          }
        }
      }
      for (int s = WAVE / 2; s > 0; s >>= 1) {
        const long long oid = __shfl_xor(best_id, s);
        const int orow = __shfl_xor(best_row, s);
        const bool mine = best_row != INT_MAX;
        const bool theirs = orow != INT_MAX;
        if (theirs && (!mine || oid > best_id ||
                       (oid == best_id && orow < best_row))) {
          best_id = oid;
          best_row = orow;
        }
      }
      // P >= 1, so lane 0 held a row and every lane now holds the winner
      newest = best_row != INT_MAX ? date[base + best_row] : INT_MIN;
    }
    const bool is_active = (long)newest > recency;
    if (!is_active) {
      for (int t = 0; t < ntiles; ++t) {
        const int r = t * WAVE + lane;
        if (r < P) keep[base + r] = 0;
      }
    }
    if (lane == 0) {
      latest[c] = newest;
      active[c] = is_active ? 1 : 0;
      if (!is_active) kept[c] = 0;
    }
  }
}

__global__ void __launch_bounds__(256)
compact_rows_kernel(const uint8_t* __restrict__ keep,
                    const long* __restrict__ kept_offset, int P,
                    int n_channels, long* __restrict__ rows,
                    int* __restrict__ row_channel) {
  const int wave = wave_id();
  const int lane = lane_id();
  const unsigned long long below = (1ULL << lane) - 1;
  const int ntiles = (P + WAVE - 1) / WAVE;

  for (int c = blockIdx.x * 4 + wave; c < n_channels; c += gridDim.x * 4) {
    const long base = (long)c * P;
    const long off = kept_offset[c];
    const long room = kept_offset[c + 1] - off;
    long running = 0;  // kept rows in the tiles before (wave-uniform)
    for (int t = 0; t < ntiles && running < room; ++t) {
      const int r = t * WAVE + lane;
      const bool k = r < P && keep[base + r] != 0;
      const unsigned long long b = __ballot(k);
      const long rank = running + __popcll(b & below);
      if (k && rank < room) {
        rows[off + rank] = base + r;
        row_channel[off + rank] = c;
      }
      running += __popcll(b);
    }
  }
}

}  // namespace crawl

extern "C" {

int crawl_channel_gate(const void* date, const void* msg_id,
                       int posts_per_channel, int n_channels, long recency,
                       void* keep, void* kept, void* active, void* latest,
                       int grid, void* stream) {
  hipLaunchKernelGGL(crawl::channel_gate_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, (const int*)date,
                     (const long*)msg_id, posts_per_channel, n_channels,
                     recency, (uint8_t*)keep, (int*)kept, (uint8_t*)active,
                     (int*)latest);
  return (int)hipGetLastError();
}

int crawl_compact_rows(const void* keep, const void* kept_offset,
                       int posts_per_channel, int n_channels, void* rows,
                       void* row_channel, int grid, void* stream) {
  hipLaunchKernelGGL(crawl::compact_rows_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, (const uint8_t*)keep,
                     (const long*)kept_offset, posts_per_channel, n_channels,
                     (long*)rows, (int*)row_channel);
  return (int)hipGetLastError();
}

}  // extern "C"
