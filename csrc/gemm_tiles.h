// The tile tables of the LDS-DMA GEMM family: ONE list of rows per family.  Each kernel file generates its launch
// switch (and so its kernel instantiations) and its ``_ok`` geometry from its list, and iit_tile_table (gemm_glds.hip)
// publishes the same rows to Python, where iit_amd/ops/hip_kernels.py checks its own tables against them at load.
// To add a tile: one row here, one row in the Python table of the same family (the load check names whichever is
// missing).  Rows stay in this order: it is the order the kernels are instantiated in.
#pragma once

// a row as iit_tile_table exports it (8 ints): bk = the K granule (K % bk == 0), ns = LDS ring depth, nw = waves,
// occ = workgroups per CU, aux = the dual families' single-launch tile id (0 elsewhere)
struct TileRow { int id, bm, bn, bk, ns, nw, occ, aux; };

// gemm_glds.hip: X(id, BM, BN, NS, NW, BK, OCC)
#define IIT_GLDS_TILE_LIST(X)                                                                                         \
  X(0, 128, 128, 3, 4, 64, 1) X(1, 128, 64, 4, 4, 64, 1) X(2, 64, 128, 4, 4, 64, 1) X(3, 64, 64, 4, 4, 64, 1)         \
  /* 8 waves (two per SIMD): 5 = 64 x 96 each, one 256-CU round for 4096 x {2304, 3072}; 6 = 32 x 64 each */          \
  X(5, 256, 192, 2, 8, 64, 1) X(6, 128, 128, 4, 8, 64, 1) X(7, 256, 128, 2, 8, 64, 1)                                 \
  /* 96 x 96: the [768][3072] / [3072][768] weight gradients are exactly 256 tiles (one per CU) where 128 x 128 */    \
  /* leaves 112 CUs idle; 2 x 2 waves of 48 x 48 (3 x 3 MFMA blocks) */                                               \
  X(8, 96, 96, 4, 4, 64, 1)                                                                                           \
  /* 128 x 96: the 4096 x 768 outputs (W_O / W_out forward, dX of QKV / W_O / W_in) are exactly 256 tiles */          \
  X(9, 128, 96, 4, 4, 64, 1)                                                                                          \
  /* 96 x 192 / 192 x 96 (2 x 2 waves of 48 x 96 / 96 x 48): the weight gradients with a 2-way reduction split */     \
  /* -- 256 workgroups for [768][3072] / [3072][768], a third fewer operand bytes per CU than 96 x 96 */              \
  X(10, 96, 192, 4, 4, 64, 1) X(11, 192, 96, 4, 4, 64, 1)                                                             \
  /* deep LDS rings (5-8 K-tiles, up to 144 KiB): more operand bytes in flight per CU for the intake-bound tiles */    \
  X(12, 96, 96, 6, 4, 64, 1) X(13, 128, 96, 5, 4, 64, 1) X(14, 64, 64, 8, 4, 64, 1)                                   \
  /* 128-deep K-tiles (256-B row segments per DMA, half the K-tiles / barriers per K): the intake experiment */       \
  X(15, 128, 96, 2, 4, 128, 1) X(16, 96, 96, 3, 4, 128, 1) X(17, 64, 64, 4, 4, 128, 1) X(18, 128, 128, 2, 4, 128, 1)  \
  /* 192 x 192 (2 x 2 waves of 96 x 96, 6 x 6 MFMA blocks): the weight gradients with a 4-way reduction split -- */    \
  /* 192 workgroups for [768][3072] / [3072][768] / 144 for [768][2304] at half the operand bytes per flop of */      \
  /* 96 x 96 (the intake-bound regime); a 2-deep ring */                                                              \
  /* (tile 19 was 192 x 192 with a 3-deep ring: wrong results under the reduction split; not offered) */              \
  /* (tile 20 serves mode 3 only: iit_gemm_glds_ok says why) */                                                       \
  X(20, 192, 192, 2, 4, 64, 1)                                                                                        \
  /* 192 x 128 / 128 x 192 (2 x 2 waves of 96 x 64 / 64 x 96), 4-deep rings (exactly 160 KiB) */                      \
  X(21, 192, 128, 4, 4, 64, 1) X(22, 128, 192, 4, 4, 64, 1)                                                           \
  /* two co-resident workgroups per CU (OCC = 2: <= 80 KiB LDS, <= 256 registers per lane), so one tile's */          \
  /* prologue / epilogue overlaps the other's main loop; shapes with >= 512 tiles */                                  \
  X(23, 128, 96, 2, 4, 64, 2) X(24, 64, 96, 3, 4, 64, 2) X(25, 128, 128, 2, 4, 64, 2)                                 \
  X(26, 96, 96, 3, 4, 64, 2) X(27, 128, 192, 2, 4, 64, 2) X(28, 64, 192, 2, 4, 64, 2)                                 \
  /* three / four co-resident workgroups per CU: the HBM-bound residual-epilogue shapes ([4096][768] outputs) */      \
  X(29, 64, 96, 2, 4, 64, 3) X(30, 64, 64, 2, 4, 64, 4) X(31, 64, 128, 2, 4, 64, 3)                                   \
  /* the in-flight-depth test on the big 8-wave tiles: 3-deep rings (2 K-tiles in flight while one is consumed, */    \
  /* tile 5 / 7 keep one) within 160 KiB, and the 256 x 256 two-stage tile */                                         \
  X(32, 256, 128, 3, 8, 64, 1) X(33, 128, 256, 3, 8, 64, 1) X(34, 256, 256, 2, 8, 64, 1)                              \
  /* (tiles 35-37, 128 / 256 x 288 for the packed-QKV forward -- 8 N-tiles of [*][2304], whole 256-CU rounds -- */    \
  /* measured 52.9-53.9 us at M = 8192 vs 39.6 us for tile 27 and 39.0 us hipBLASLt, and the 2-deep 128 x 288 */      \
  /* returned NaNs (profiles/qkv_fwd_tiles_r4.txt): removed; not offered) */                                          \
  X(4, 128, 128, 4, 4, 64, 1) /* tile 0 with a 4-deep ring */
// The 256 x 256 kernels that share the glds tile ids but have launch paths of their own (published, not launched from
// the list): 40 = the 8-phase kernel of gemm_8ph.hip, 41 / 42 = the four-wave kernel of gemm_4w.hip with 64- / 32-deep
// K-tiles in a 2- / 4-slot ring.  BK is the K granule iit_gemm_8ph_ok asks of all three; each file asserts its row.
#define IIT_GLDS_BIG_TILE_LIST(X) X(40, 256, 256, 2, 8, 64, 1) X(41, 256, 256, 2, 4, 64, 1) X(42, 256, 256, 4, 4, 64, 1)

// gemm_edge.hip, the edge-capable tiles under their glds ids: X(id, BM, BN, NS, NW, OCC)
#define IIT_EDGE_TILE_LIST(X) X(0, 128, 128, 3, 4, 1) X(7, 256, 128, 2, 8, 1) X(25, 128, 128, 2, 4, 2)

// gemm_dual.hip: X(idx, BM, BN, NS, NW, OCC, glds_id); glds_id = the single-launch tile of the same BM x BN whose
// shape checks the pair borrows (its ring depth / occupancy may differ).  A dW and a dX tile share a launch exactly
// when their (NW, OCC) are equal -- three families (W 0-4 / X 0-3, W 5-6 / X 4-6, W 7-8 / X 7-8):
// * 4 waves, two workgroups per CU: one problem's prologue / epilogue under the other's main loop on the same CU;
// * 8 waves (two per SIMD), one workgroup per CU: the big tiles that run the paired forward at ~1 PF/s (fewer operand
//   bytes per flop than 128x128), which alone leave most of the CUs idle on a [768][N] weight gradient; here the dX
//   tiles fill them.  (A 256x192 dW tile spills registers: not offered.)
// * 4 waves, one workgroup per CU, deep rings (3-4 K-tiles, up to 128 KiB): more operand bytes in flight for the
//   operands that come cold from HBM inside the step (the activations saved by the forward), where the two-stage
//   rings of the two-per-CU tiles wait on the fill.
#define IIT_DUAL_W_TILE_LIST(X)                                                                                  \
  X(0, 128, 96, 2, 4, 2, 23) X(1, 128, 128, 2, 4, 2, 25) X(2, 96, 96, 3, 4, 2, 26) X(3, 64, 96, 3, 4, 2, 24)     \
  X(4, 64, 64, 4, 4, 2, 3)                                                                                       \
  X(5, 256, 128, 2, 8, 1, 7) X(6, 128, 128, 4, 8, 1, 6)                                                          \
  X(7, 128, 128, 4, 4, 1, 4) X(8, 128, 96, 4, 4, 1, 13)
#define IIT_DUAL_X_TILE_LIST(X)                                                                                  \
  X(0, 128, 96, 2, 4, 2, 23) X(1, 64, 96, 3, 4, 2, 24) X(2, 128, 192, 2, 4, 2, 27) X(3, 128, 128, 2, 4, 2, 25)   \
  X(4, 256, 192, 2, 8, 1, 5) X(5, 256, 128, 2, 8, 1, 7) X(6, 128, 128, 4, 8, 1, 6)                               \
  X(7, 128, 128, 4, 4, 1, 4) X(8, 128, 192, 3, 4, 1, 22)

// conv_nhwc.hip, forward / input gradient: X(id, BM, BN, NS, NW, OCC); the output is [N H W][Cout] with Cout 64..512
#define IIT_CONV_TILE_LIST(X)                                                 \
  X(0, 128, 64, 4, 4, 1) X(1, 128, 128, 3, 4, 1) X(2, 64, 64, 4, 4, 2)        \
  X(3, 128, 128, 2, 4, 2) X(4, 64, 128, 2, 4, 3) X(5, 128, 64, 2, 4, 2)
// conv_nhwc.hip, weight gradient: X(id, BM = Cout rows, BN = channels of one tap, NS); 4 waves, one workgroup per CU
#define IIT_CONV_WG_TILE_LIST(X) X(0, 64, 64, 4) X(1, 128, 64, 4) X(2, 128, 128, 3) X(3, 64, 128, 4)

#define IIT_ROW_GLDS(ID, BM, BN, NS, NW, BK, OCC) {ID, BM, BN, BK, NS, NW, OCC, 0},
#define IIT_ROW_K64(ID, BM, BN, NS, NW, OCC) {ID, BM, BN, 64, NS, NW, OCC, 0},
#define IIT_ROW_DUAL(ID, BM, BN, NS, NW, OCC, GLDS) {ID, BM, BN, 64, NS, NW, OCC, GLDS},
#define IIT_ROW_WG(ID, BM, BN, NS) {ID, BM, BN, 64, NS, 4, 1, 0},
constexpr TileRow kGldsRows[] = {IIT_GLDS_TILE_LIST(IIT_ROW_GLDS) IIT_GLDS_BIG_TILE_LIST(IIT_ROW_GLDS)};
constexpr TileRow kEdgeRows[] = {IIT_EDGE_TILE_LIST(IIT_ROW_K64)};
constexpr TileRow kDualWRows[] = {IIT_DUAL_W_TILE_LIST(IIT_ROW_DUAL)};
constexpr TileRow kDualXRows[] = {IIT_DUAL_X_TILE_LIST(IIT_ROW_DUAL)};
constexpr TileRow kConvRows[] = {IIT_CONV_TILE_LIST(IIT_ROW_K64)};
constexpr TileRow kConvWgRows[] = {IIT_CONV_WG_TILE_LIST(IIT_ROW_WG)};

// the row of tile ``id``, or nullptr: no such tile
template <int N>
constexpr const TileRow* find_tile(const TileRow (&rows)[N], int id) {
  for (int i = 0; i < N; ++i)
    if (rows[i].id == id) return &rows[i];
  return nullptr;
}

// an edge tile is the glds tile of the same id, ring and occupancy included; a dual tile's glds_id has its BM x BN
constexpr bool same_tile(const TileRow& r, const TileRow* g, bool ring) {
  return g && g->bm == r.bm && g->bn == r.bn && g->bk == r.bk &&
         (!ring || (g->ns == r.ns && g->nw == r.nw && g->occ == r.occ));
}
constexpr bool tile_lists_agree() {
  for (const TileRow& r : kEdgeRows)
    if (!same_tile(r, find_tile(kGldsRows, r.id), true)) return false;
  for (const TileRow& r : kDualWRows)
    if (!same_tile(r, find_tile(kGldsRows, r.aux), false)) return false;
  for (const TileRow& r : kDualXRows)
    if (!same_tile(r, find_tile(kGldsRows, r.aux), false)) return false;
  return true;
}
static_assert(tile_lists_agree(), "gemm_tiles.h: an edge or dual row disagrees with the glds row it names");
