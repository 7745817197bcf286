// solver_layout.h — what the host's launch planner (host/solver_plan.cc) and the solver kernels agree on: the LDS
// carve-ups, the layouts of the buffers the workgroups exchange rows through, and the instantiated block sizes of every
// kernel family.  Constants and integer functions only: no HIP include, no device code (the solver's model_layout.h).
#pragma once

#ifdef __HIPCC__
#define IDTO_LAYOUT_HD __host__ __device__
#else
#define IDTO_LAYOUT_HD
#endif

// ---- The instantiations, one list per kernel family: X(...) per entry.  The hipFuncSetAttribute block, the dispatch
// switches (idto_hip.hip) and the planner's "is this size instantiated" tests (SolverInstantiated below) all expand these.
// penta_ldl_kernel<K, 256, PD, GW>: X(K, padded, elimination wavefronts)
#define IDTO_LDL_KERNELS(X) \
  X(2, false, 1) X(3, false, 1) X(5, false, 1) X(19, false, 1) X(23, false, 2) X(8, true, 1) X(16, true, 1) X(24, true, 2) \
  X(30, true, 2) X(29, false, 2) X(4, false, 1) X(32, true, 3)
// penta_nd_kernel<K, false>
#define IDTO_ND_KERNELS(X) X(2) X(3) X(5) X(19) X(23) X(29) X(8)
// penta_pipe_kernel<K> ...
#define IDTO_PIPE_KERNELS(X) X(2) X(3) X(5) X(19)
// ... and penta_pipe_kernel<K, true>, the launches that also decide on the trust-region loop's trial point
#define IDTO_PIPE_DEC_KERNELS(X) X(5) X(19)
// penta_band_kernel<W>, W = 3 k
#define IDTO_BAND_KERNELS(X) X(6) X(9) X(12) X(15)
// penta_apply_kernel<K, K <= 8> (and penta_factor_transpose_kernel<K> in front of the large ones)
#define IDTO_APPLY_KERNELS(X) X(2) X(3) X(5) X(8) X(16) X(19) X(23) X(24) X(32)
// gn_fused_kernel<MAXC, K, PD, GW>
#define IDTO_FUSED_KERNELS(X) X(2, 2, false, 1) X(3, 3, false, 1) X(3, 5, false, 1) X(3, 19, false, 1) X(4, 23, false, 2)
// gn_small_kernel<SHAPE, W, 256, WS, TR>: X(SHAPE, W, WS, TR) - the plain step, the trust-region loop's, with one enforced constraint
#define IDTO_SMALL_KERNELS(X) X(1, 6, 6, false) X(5, 9, 9, false) X(1, 6, 6, true) X(5, 9, 9, true) X(1, 6, 9, true) X(5, 9, 12, true)

namespace idto_dev {

enum SolverFamily { FAM_LDL, FAM_ND, FAM_PIPE, FAM_PIPE_DEC, FAM_BAND, FAM_APPLY };
// is size `v` (block size; the band kernel: W) in the family's list?
constexpr bool SolverInstantiated(SolverFamily f, int v) {
#define IDTO_X1(K) || v == K
#define IDTO_X3(K, PD, GW) || v == K
  switch (f) {
    case FAM_LDL: return false IDTO_LDL_KERNELS(IDTO_X3);
    case FAM_ND: return false IDTO_ND_KERNELS(IDTO_X1);
    case FAM_PIPE: return false IDTO_PIPE_KERNELS(IDTO_X1);
    case FAM_PIPE_DEC: return false IDTO_PIPE_DEC_KERNELS(IDTO_X1);
    case FAM_BAND: return false IDTO_BAND_KERNELS(IDTO_X1);
    case FAM_APPLY: return false IDTO_APPLY_KERNELS(IDTO_X1);
  }
  return false;
#undef IDTO_X1
#undef IDTO_X3
}

// ---- penta_ldl.h

// Column stride (in doubles) of every K-row block kept in LDS and of the row-major factor blocks:
// even (16-byte aligned columns for ds_read_b128), = 2 mod 4, i.e. an odd number of 16-byte
// units, so that consecutive columns start in different LDS bank groups, and >= 4 ceil(K/4): the
// MFMA k-steps read rows up to 4 ceil(K/4) - 1 of a column (zero pad rows).
IDTO_LAYOUT_HD constexpr int ldl_ks(int K) { return 4 * ((K + 3) / 4) + 2; }

struct PentaLdlLds {  // offsets in doubles
  int W, Ht, Et, Iv, rt, U, G, in, dump, yh, ye, Eb, bl, bl_size, xall, end;
  int kks, rts;
};
// `rows` (> 0, single right-hand side): the chain's local rows incl. pseudo-rows - the right-hand side and rt / x of
// every row are indexed by LOCAL row, so a workgroup of the two-sided elimination needs its own half only
IDTO_LAYOUT_HD inline PentaLdlLds penta_ldl_layout(int n, int K, int nrhs, int rows = 0) {
  PentaLdlLds L;
  const int ks = ldl_ks(K), ncr = 2 * K + nrhs;
  L.kks = K * ks;
  L.rts = nrhs * ks;
  int o = 0;
  L.W = o; o += (K + ncr) * ks;   // augmented block [S | H | E | y], column-major, stride ks
  L.Ht = o; o += 2 * L.kks;       // ring: Ht_i, Ht_{i-1}
  L.Et = o; o += 3 * L.kks;       // ring: Et_i, Et_{i-1}, Et_{i-2}
  L.Iv = o; o += 3 * ks;          // ring: 1/diag(U) (padded to ks)
  L.rt = o; o += 3 * L.rts;       // ring: rt_i (forward) / x_i (backward)
  L.U = o; o += 2 * L.kks;        // ring: U_i, U_{i-1} (write-back staging)
  L.G = o; o += (K * K + 1) & ~1; // Et_{i-1}^T Dn Et_{i-1} for the next row (even size: what follows is read as double2;
                                  // b128 reads off a 16-byte boundary halve the LDS throughput)
  {                               // staged A_i, B_{i+1}, C_i, A_{i+2}; reused by the backward pass
    const int fwd = 4 * K * K, bwd = 3 * K * ks + ks;
    L.in = o; o += ((fwd > bwd ? fwd : bwd) + 1) & ~1;
  }
  L.dump = o; o += 2;             // write target of staging lanes without a slot
  L.yh = o; o += 2 * ks;          // y-push rings: (Ht_i^T Dn rt_i) of the last two rows ...
  L.ye = o; o += 3 * ks;          // ... and (Et_i^T Dn rt_i) of the last three
  L.Eb = o; o += 2 * L.kks;       // E_i = A_{i+2}^T staged straight in column layout (row parity)
  L.bl = o;
  const int nr = (rows > 0 && nrhs == 1 && rows < n) ? rows : n;
  L.bl_size = (nrhs * n * K <= 4096) ? nrhs * nr * K : 0;
  o += (L.bl_size + 1) & ~1;      // right-hand sides staged in LDS when small ...
  L.xall = o;                     // ... and rt_i / x_i of every row: [j][n + 2][ks], two leading zero rows
  o += L.bl_size ? nrhs * (nr + 2) * ks : 0;
  L.end = o;
  return L;
}

// local rows (incl. the producer's two pseudo-rows, + 2 spare) either workgroup of the two-sided kernel touches
IDTO_LAYOUT_HD inline int ldl_two_sided_rows(int n, int m_split, int nrhs) {
  if (m_split <= 0 || nrhs != 1) return 0;
  const int top = m_split + 2, bottom = n - m_split;
  return (top > bottom ? top : bottom) + 2;
}

// ---- penta_nd.h

enum { ND_MAXROWS = 32 };  // local rows of a joiner chain (incl. its two join rows)

struct NdBuf { int rtpub, fst, frow, xsep, ll, joinll, joinll_pair, end; };  // offsets in doubles; rtpub / fst are [2][...]
IDTO_LAYOUT_HD inline NdBuf nd_layout(int K) {
  NdBuf L;
  const int ks = ldl_ks(K), ct2 = (2 * K + 1 + 15) / 16;   // columns [Ft | rt], in tiles of 16
  int o = 0;
  L.rtpub = o; o += 2 * ND_MAXROWS * K;
  L.frow = 16 * ct2 * ks;                // doubles per published row (whole 16-column tiles: the separator's MFMA loads)
  L.fst = o; o += 2 * ND_MAXROWS * L.frow + 16 * ks;
  L.xsep = o; o += 2 * K;
  o += o & 1;
  L.ll = o; o += 3 * 4 * K;              // flagged copies (ll_store): x_sep, and the two join rows of each producer / joiner pair
  L.joinll = o; L.joinll_pair = 2 * 2 * K * 64;            // [pseudo row][r][column: 64 lanes] of 16-byte slots   // penta_pipe.h: a producer's Schur-complement contributions to the join rows, flagged
  o += 2 * L.joinll_pair;
  L.end = o;
  return L;
}

// doubles of the separator's Q: per spike workgroup the lower-triangle tiles of Q as the matrix cores leave them
// ([tile][register][lane]: stored and summed without a condition or a transposed copy)
IDTO_LAYOUT_HD constexpr int nd_sep_q_tiles(int K) { return ((2 * K + 1 + 15) / 16) * ((2 * K + 1 + 15) / 16 + 1) / 2; }
IDTO_LAYOUT_HD constexpr int nd_sep_q_doubles(int K) { return 2 * nd_sep_q_tiles(K) * 256; }
// (the whole carve-up of nd_separator)
IDTO_LAYOUT_HD inline int nd_sep_lds_doubles(int K) {
  const int ks = ldl_ks(K);
  return nd_sep_q_doubles(K) + (2 * K + 1) * ks + (K + 1) * ks + 2 * K * ks + K * ks + 4 * ks + 2;
}

// ---- penta_band.h

// The split and the LDS carve-up (doubles).  First chain: pivots 0 .. m - 1 (m a multiple of W), then the W middle rows
// m .. lim - 1 (three whole blocks; w would do); mirrored chain: the nb rows behind them in the order band_mirror
// gives them, `pad` identity pivots in front.  Columns of a copy: FRONT zero columns (the back substitution's reads
// above row 0 and its blocks of four steps run into them), the chain's own, 2 W + 1 padding columns (identity behind the first chain's, zero behind
// the mirrored chain's: those only collect its Schur complement).
struct BandLds { int m, lim, nb, pad, tcols, bcols, T, Bm, Dt, Db, D0, J, end; };
constexpr int BAND_FRONT = 32;
IDTO_LAYOUT_HD inline BandLds band_layout(int M, int W) {
  BandLds L;
  L.m = ((M - W) / 2 + W / 2) / W * W;
  L.lim = L.m + W;
  L.nb = M - W - L.m;
  L.pad = (W - L.nb % W) % W;
  L.tcols = BAND_FRONT + L.lim + 2 * W + 1;
  L.bcols = BAND_FRONT + L.pad + L.nb + 2 * W + 1;
  int o = 0;
  L.T = o; o += L.tcols * 16;
  L.Bm = o; o += L.bcols * 16;
  L.Dt = o; o += L.tcols;
  L.Db = o; o += L.bcols;
  L.D0 = o; o += M + (M & 1);   // the diagonal entries as assembled (pivot test)
  L.J = o; o += W * 16;   // the mirrored chain's window at the join, [slot][lane]
  L.end = o;
  return L;
}

// ---- penta_pipe.h

// positions (in doubles) inside one published row; every part starts at an even position so that pairs are
// 16-byte aligned for ds_read_b128
template <int K>
struct PipeGeo {
  static constexpr int KE = K + (K & 1);
  static constexpr int KR = 4 * ((K + 3) / 4);        // rows of a ring slot (pad rows stay zero: MFMA k-steps)
  static constexpr int oS = 0, oH = KE, oE = 2 * KE, oy = 3 * KE, oF = 3 * KE + 2;
  static constexpr int od = oF + 2 * K;               // the main wavefront's "row published" word (NaN until then)
  static constexpr int og = od + 1;                   // the spike wavefront's
  static constexpr int oi = og + 1;                   // 1 / d_j
  static constexpr int odump = oi + 1;                // 8 positions written by lanes that hold no column
  static constexpr int oz = odump + 8;                // a position that stays zero
  // the parts the follower multiplies with, once more UNscaled: W_{i+1}[r][c] -= (Ht[j][r] / d_j) * Ht[j][c] with the
  // second factor as it sits in the eliminating wavefront's registers (recomputing it as scaled * d costs two more
  // roundings per term: measurably less accurate at cond(H) ~ 1e12)
  static constexpr int oRH = oz + 1 + ((oz + 1) & 1), oRE = oRH + KE, oRy = oRE + KE;
  static constexpr int used = oRy + 1;
  static constexpr int RS = ((used + 15) / 32) * 32 + 16;   // = 16 mod 32: the four k-rows of an MFMA operand read hit different banks
  static constexpr int SLOT = KR * RS;
  static constexpr int GS = ldl_ks(K);                // column stride of the staged inputs and of G
  static constexpr int NCX = 3 * K + 1;               // columns [S | H | E | y] of the main wavefront
  static constexpr int NGC = KE + 2 + 2 * K;          // columns of G: [S-part (K, padded to KE) | y | . | F (2K)]
  static_assert(3 * K <= 61, "main wavefront: 3K + 1 columns and the lane that publishes d");
  static_assert(RS >= used && RS % 32 == 16, "row stride");
};

// The follower that eliminates next ("low" follower) takes rows 0 .. RLO-1 of the next block row, the wavefront that
// has just eliminated takes the rest and hands them over through LDS (PipeRows below).  K >= 17: RLO = 16, ONE row tile
// of the matrix cores - the low follower forms Ht^T Dn [Ht | Et | rt] (spike wavefronts: Ht^T Dn Ft) for its 16 rows
// with v_mfma_f64_16x16x4, a k-step per four published pivots (pipe_follow_mfma), instead of K rank-one updates
// with broadcast multipliers.
template <int K>
constexpr int pipe_rlo() { return K >= 17 ? 16 : (K >= 3 ? (((K + 1) / 2 + 1) & ~1) : K); }
template <int K>
constexpr bool pipe_mfma_follow() { return K >= 17; }
// the low follower's products leave the matrix cores as tiles (lane = (k-row, column), register = row); the wavefront
// turns them into its own layout (lane = column, register = row) through a scratch of its own: PIPE_HPC product columns
// (three column tiles) + one column that stays zero (lanes whose column takes no update), column stride PIPE_HS (16 rows;
// 36 dwords: eight lanes' 16-byte reads cover the 32 banks once)
constexpr int PIPE_HPC = 48, PIPE_HS = 18, PIPE_HPN = (PIPE_HPC + 1) * PIPE_HS;

struct PipeLds {   // offsets in doubles
  int ring, stage, gbuf, xhi, hp, jbuf, xall, W, flags, end;
};
template <int K>
IDTO_LAYOUT_HD inline PipeLds pipe_layout(int n, bool spike) {
  using G = PipeGeo<K>;
  PipeLds L;
  int o = 0;
  L.ring = o; o += 3 * G::SLOT;
  // (the main columns only: the spike wavefronts take their first two rows' inputs straight from the band arrays.
  // Rounds 3-5 reserved 2 x 2K more columns here that nothing wrote or read: 12 KB at K = 19)
  L.stage = o; o += 2 * G::NCX * G::GS + 2;   // (+ a dump double)
  L.gbuf = o; o += 2 * G::NGC * G::GS;
  {   // the second follower's rows of the next block row, [column][row] (+ a dump column)
    constexpr int NHI = K - pipe_rlo<K>();
    L.xhi = o; o += (G::NCX + (spike ? 2 * K : 0) + 1) * (NHI + (NHI & 1)) + 2;
  }
  L.hp = o; o += pipe_mfma_follow<K>() ? (spike ? 2 : 1) * PIPE_HPN : 0;   // pipe_follow_mfma's scratch: main wavefronts, spike wavefronts
  (void)n;
  L.jbuf = o; o += spike ? (3 * K + 2) * G::KE : 0;   // a joiner: the producer's contributions to its two join rows, columns [S | H | y], [S | y]
  L.xall = o; o += (ND_MAXROWS + 2) * G::GS;   // rt of the chain's local rows (two leading zero rows)
  L.W = o; o += 2 * G::KE + 2;
  L.flags = o; o += 32;            // 64 ints
  L.end = o;
  return L;
}

// The back substitution in recursion form (penta_pipe.h pipe_backward).
// LDS (everything the forward pass used is free): per local row [Y | Z] row-major (stride 2 KE), W likewise, c.
template <int K, bool SPK>
struct PipeBack {
  // (a row-major block also stages D^-1 U, stride ks.  Row stride: not a multiple of 16 dwords, or the rows that the
  // lanes of the recursion read - one row per lane, ds_read_b128 - start in 2 (K = 23: 96 dwords) or 4 (K = 19: 80) of the
  // 16 bank groups; K = 29: 120 dwords, 8 groups, left alone - two more doubles per row and 11 rows of the KKT system
  // at N = 40 no longer fit)
  static constexpr int KE = K + (K & 1), YS0 = 2 * KE > ldl_ks(K) ? 2 * KE : ldl_ks(K), YS = YS0 + (YS0 % 8 == 0 ? 2 : 0);
  static constexpr int oYZ = 0, oW = K * YS, oC = oW + (SPK ? K * YS : 0), BS = oC + KE;
};

// A producer's recursion in closed form (penta_pipe.h pipe_closed_build): behind its rows of [Y | Z | c], the x ring and
// the dump, per local row T_i = [G_i | chat_i] with x_i = chat_i + G_i [x_nloc ; x_nloc+1] - K rows of 2 KE + 1 entries,
// the columns laid out like the two join rows in the x ring (pad columns zero) - and the identity in two more slots.
// (Row stride: even, and no multiple of 16 dwords - the last pass reads a row per lane, as the recursion does.)
template <int K>
struct PipeClosed {
  using B = PipeBack<K, false>;
  static constexpr int KE = B::KE, NC = 2 * KE + 1, TS0 = 2 * KE + 2, TS = TS0 + (TS0 % 8 == 0 ? 2 : 0), SLOT = K * TS;
  static constexpr int PAR = 8 * 2 * KE;   // behind the wavefronts' copies of the join rows, in what held rt of the local rows: seven words of arguments
  IDTO_LAYOUT_HD static constexpr int base(int nloc) { return nloc * B::BS + 4 * KE + 2; }
  IDTO_LAYOUT_HD static constexpr int end(int nloc) { return base(nloc) + (nloc + 2) * SLOT; }
};

// ---- the seven-workgroup kernel's chains (penta_nd.h, K = 23 / 29) take their back substitution in the same form.
// Their forward pass (penta_ldl_body) leaves rt of the local rows at xall_off, in the middle of what the recursion
// matrices will occupy: the rows move to the top of the launch's LDS first.
// -> the number of the producer's wavefronts that work on the partner's rows (each stages a block D^-1 U of its own), 0: does not fit
template <int K>
IDTO_LAYOUT_HD inline int pipe_recursion_tail_fits(int lds_doubles, int nloc_joiner, int nloc_producer) {
  using B = PipeBack<K, false>;
  constexpr int ks = ldl_ks(K);
  const int nloc = nloc_joiner > nloc_producer ? nloc_joiner : nloc_producer;
  if (!(nloc_joiner * B::BS + 6 * B::KE + 4 <= lds_doubles - (nloc_joiner + 2) * ks && (nloc + 2) * ks <= 4 * 256 &&
        nloc_joiner * K <= 2 * 256))
    return 0;
  for (int w = 4; w >= 1; w >>= 1)
    if (nloc_producer * B::BS + 6 * B::KE + 4 + w * K * ks <= lds_doubles - (nloc_producer + 2) * ks) return w;
  return 0;
}

// ---- gn_small.h

// LDS of the folded iteration (doubles); it has to fit the band solver's carve-up (the host checks)
IDTO_LAYOUT_HD constexpr int gn_small_fold_doubles(int N, int K) { return 26 * (N + 1) * K + 18 * (N + 1) + 32; }

// doubles of dynamic LDS behind the band solver's carve-up (gn_small_kernel's own arrays, in its order)
IDTO_LAYOUT_HD inline int gn_small_doubles(int N, int K, int fast_n, int KK = 0) {
  const int E = 1 + 3 * K;
  if (KK > K) return gn_small_doubles(N, K, fast_n) + 3 * (N + 1) * KK * KK + (N + 1) * KK;
  return 2 * (N + 1) * K + N * K + 3 * N * E + N * E * K + K * K + 3 * N * K * K + 5 * K + (K & 1) + fast_n + (fast_n & 1) +
         3 * (N + 1) * K * K + 3 * (N + 1) * K + 2 * K * K + (K * K & 1) + K + 2 +
         5 * K + (K & 1) + (3 * N + 2) * (K + 1) + 2 * (N + 1) + 2 + 24;   // (the trust-region loop's cost and decision)
}

}  // namespace idto_dev
