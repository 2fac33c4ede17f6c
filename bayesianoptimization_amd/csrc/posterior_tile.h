// What the posterior's four MFMA GEMM kernels share (posterior_kernel_v2, posterior_kernel_f32, posterior_kernel_f32x,
// posterior_i8_kernel): the grid of (row chunk of W, 64-candidate tile) workgroups with its block map, and the buffer
// descriptor word their operand loads use.
#pragma once

#include <cstdint>

namespace gpbo {

constexpr int BUF_FLAGS = 0x00020000;   // gfx9 buffer descriptor word 3: raw buffer, 32-bit data format

// One launch: nchunks row chunks of W x n_ctiles tiles of 64 candidates, a workgroup each.  Embedded in the kernels' argument
// structs where these four fields already lay.
struct PostGrid {
  int NP;
  int64_t Mp;        // row pitch of the partials `part` [nchunks][Mp]
  int nchunks;
  int n_ctiles;

  int64_t blocks() const { return (int64_t)n_ctiles * nchunks; }

  // Heaviest row chunks first (W is lower triangular: chunk r multiplies r + 1 chunks of columns); the workgroups resident at
  // any time share a chunk, so its rows of W come out of L2.
  // (Round-2 A/B on the fp64 kernel: mappings that put the two chunks of a candidate tile 1 ... 64 block ids apart, hoping the
  // second chunk's k* reads would hit the first one's in L2, never lowered FETCH_SIZE — 3.5e11 ... 6.6e11 B against 3.3e11 — and
  // cost up to 6 % of the time; removed.  Int8 kernel, candidate tile outermost instead, so that the row chunks of a tile share
  // its k* digits in L2: 283 ms per C3 pass against 196, with 256 MB ... 4 GB slabs alike.)
  __device__ __forceinline__ void map(int bid, int& r, int& ct) const {
    r = nchunks - 1 - bid / n_ctiles;
    ct = bid - (bid / n_ctiles) * n_ctiles;
  }
};

}  // namespace gpbo
