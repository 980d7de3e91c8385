// Where an entry of a solve tile's panel lives (kernels.h: SpdItem).  Shared by everything that lays panels out (the host
// packer of SpdSolverDev::upload, k_pack_panels) and by the streaming loop that reads them (kernels.hip: stream_rest).
//
// A tile's lane (r, kq), KQ = 64 / rows lanes per row, consumes the entries k = kq, kq + KQ, kq + 2 KQ, ... of its row r.
//   plain  (pair_kq == 0):  entry (k, r) at k * ld + r: one double per lane and load
//   paired (pair_kq == KQ): the two entries a lane consumes one after the other are neighbours, so one 16-byte load
//                           fetches both and a wave's load covers 1 KiB contiguous: for k = g * 2 KQ + h * KQ + kq,
//                           h in {0, 1}, entry (k, r) at ((g * KQ + kq) * ld + r) * 2 + h.  The panel's length in k is
//                           rounded up to a multiple of 2 KQ; the pad entries are zero and never multiplied.
// Groups of 2 KQ entries never straddle a chunk of the reduction (spd_chunk: chunk starts are multiples of 8) for KQ = 1
// and 4; the 8-row root class (KQ = 8) keeps the plain layout.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPD_PANEL_HD __host__ __device__
#else
#define SPD_PANEL_HD
#endif

namespace dpgo {

// lanes per row of the class with `rows`-high tiles if its panels are paired, 0 if they are plain
SPD_PANEL_HD inline int spd_pair_kq(bool pairs, int rows) { return (pairs && (rows == 64 || rows == 16)) ? 64 / rows : 0; }
// doubles between consecutive rows of a panel of a tile with `count` rows (8-row tiles: a wave's load spans 8 consecutive
// 64-byte rows)
SPD_PANEL_HD inline int spd_panel_ld(int rows, int count) { return rows == 8 ? 8 : (count + 15) / 16 * 16; }
// rows of ld doubles a panel of `len` entries per row takes
SPD_PANEL_HD inline int64_t spd_panel_len(int pair_kq, int64_t len) {
  return pair_kq ? (len + 2 * pair_kq - 1) / (2 * pair_kq) * (2 * pair_kq) : len;
}
// offset of entry (k, r) from the panel's start, in doubles
SPD_PANEL_HD inline int64_t spd_panel_index(int pair_kq, int ld, int64_t k, int r) {
  if (!pair_kq) return k * ld + r;
  const int64_t g = k / (2 * pair_kq);
  const int rem = (int)(k - g * 2 * pair_kq), h = rem / pair_kq, q = rem - h * pair_kq;
  return ((g * pair_kq + q) * ld + r) * 2 + h;
}

}  // namespace dpgo
