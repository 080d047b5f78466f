// Weight-gradient GEMM for all six layers in ONE launch (grouped, split-K over the batch).
//
//   dW_aug[n][k] = sum_m dY[m][n] * X[m][k]      (k == K is the bias column: X^T row K == 1)
//
// Both operands are feature-major (written transposed by mlp_train_kernel), so every MFMA
// fragment is one 16-byte load along m, the reduction axis.  A task = (layer, output tile,
// batch chunk).  The tile is nq x kq QUADRANTS of 64x64 (nq * kq <= 8, nq + kq <= 6), one per
// wave of the 8-wave workgroup, or at split-bf16 / bf16 up to 16 quadrants, two per wave
// (wgrad_task_ok); each quadrant = 4x4 MFMA tiles of 16x16 (64 f32 accumulator registers).  The host plan picks (nq, kq) per layer to minimise operand rows read per
// k-step: the kernel is bound by the operand stream (HBM / MALL), and a 256x128 tile reads
// 384 rows per step for 2x the outputs of a 128x128 tile's 256 (v_fc1: 2304 instead of 3072
// rows per step).  Results go to per-chunk fp32 slabs ([nq*64][kq*64] per task) that
// grad_gather sums in a fixed order — deterministic, no float atomics (SURVEY §7.4 part 2).
#include <type_traits>

#include "kernels.h"
#include "mlp_core.h"

namespace {

constexpr int WG_WAVES = 8;

// The workgroup stages each k-step's distinct fragments (4*nq of dY^T, 4*kq of X^T) ONCE into
// LDS with LDS-DMA (global_load_lds_dwordx4): an FM fragment is 64 lanes x 16 B per KiB in lane
// order, exactly the lane-linear image the DMA writes, so the fragment reads are conflict-free
// ds_read_b128 at lane*16.  A split-bf16 fragment (32 B per lane: hi | lo) is two DMA
// instructions, instruction h moving the fragment's h-th KiB (lanes 32h .. 32h+31) so it lands
// as [their hi][their lo] (the dense layout of mlp_stream.hip frag_lane_off).  Each wave DMAs C
// fixed slots per stage (C = 2 when the task has <= 16 fragments, 3 <= 24, 4 <= 32, 5 <= 40; slots past the task's
// fragment count re-load one of its fragments, an L2 hit, so every wave's DMA count — and with
// it the vmcnt arithmetic — is task-independent).  S-deep ring, counted vmcnt and a raw
// s_barrier keep S-1 steps of DMA in flight across the barrier (cdna_hip_programming.md
// 'Pipelining across barriers'): no VGPRs hold in-flight data.
// bytes per operand slot: one fragment (32 batch rows of 16 features); e4m3 (DT_FP8) four
// fragments of consecutive k-steps (128 batch rows, 2 KiB: two DMA instructions; they are
// contiguous in the FM layout), one v_mfma_scale_f32_16x16x128_f8f6f4 per tile pair — twice the
// bf16 MFMA rate — so a kernel "k-step" there covers 128 rows
template <int DT>
constexpr int wgrad_frag_bytes() { return DT == DT_FP8 ? 2048 : 512 * Prec<DT>::BYTES; }
template <int DT>
constexpr int wgrad_step_rows() { return DT == DT_FP8 ? 128 : 32; }
typedef __attribute__((ext_vector_type(8))) int i32x8;

// the 16-byte chunk swizzle of a row-major operand image (128-byte rows): even XOR values keep the two
// chunks of a 16-feature column group adjacent; rows r, r + 2, r + 8, r + 10 (the rows of a 32-lane
// half's transposed reads that share banks) get distinct chunk pairs — conflict-free
__host__ __device__ inline int wgrad_swz(int row) { return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2); }

// Row-major operands: lane l's MFMA operand (feature 16 s + (l & 15) of a quadrant, rows 8 (l >> 4)
// .. + 7) is two ds_read_b64_tr_b16 of 4 rows each (lane 4 q' + p' of a 16-lane group addresses row
// q', columns 4 p' .. 4 p' + 3; lane i receives column i) per precision part.  rm_off: the byte
// offset (within a stage) of read `sub` of slot f (quadrant slots f & ~3 .. + 3, s = f & 3)
DEV unsigned rm_off(int f, int sub, int lane, int FB) {
  const int li = lane & 15, g = lane >> 4;
  const int row = 8 * g + 4 * sub + (li >> 2), col = 16 * (f & 3) + 4 * (li & 3);
  return (unsigned)((f & ~3) * FB + row * 128 + (((col >> 3) ^ wgrad_swz(row)) << 4) + (col & 7) * 2);
}
// Split-bf16 row-major quadrants keep the memory's [8 hi | 8 lo] groups: a row's 64 features are 256
// contiguous bytes, DMA'd 4 rows per instruction (16 lanes x 16 B per row: whole 256-byte row
// segments, not 16-byte pieces at a 32-byte stride), the 16 chunks of a row XOR-swizzled by
// wgrad_swz16(row) so the 16 rows of a transposed read meet each 16-byte bank group at most twice
// (the 2-cycle minimum of a 512-byte read)
__host__ __device__ inline int wgrad_swz16(int row) { return ((row & 3) << 2) | ((row >> 3) & 3); }
// (rmask 31: the 32-row quadrant image of a full stage; 15: the 16-row image of a half-stage unit,
// the lane's half (lane >> 5) choosing the unit — the swizzle stays that of the full row)
DEV unsigned rm_off_s3(int f, int sub, int part, int lane, int FB, int rmask = 31) {
  const int li = lane & 15, g = lane >> 4;
  const int row = 8 * g + 4 * sub + (li >> 2), col = 16 * (f & 3) + 4 * (li & 3);
  const int pos = ((col >> 3) * 2 + part) ^ wgrad_swz16(row);
  return (unsigned)((f & ~3) * FB + (row & rmask) * 256 + pos * 16 + (col & 7) * 2);
}
// Split-bf16 / bf16 fragment reads (common.h: inline-asm LDS reads the compiler neither waits for
// nor drains the DMA ring for; with the ds_read_tr16_b64 builtin it put s_waitcnt vmcnt(0) in front
// of every row-major read, and a runtime layout branch made each read a basic block of its own
// with its own lgkmcnt(0): docs/ARCHITECTURE.md §15).  The operand layout is a template parameter
// of the loop body; a fragment's reads land in a WgRaw — row-major: two 4-row transposed reads per
// precision part (hi sub 0, hi sub 1 [, lo sub 0, lo sub 1]; the second 4 rows are an instruction
// offset: neither swizzle looks at row bit 2), fragment-major: one ds_read_b128 per part — and
// become the MFMA operand only after the group's settle (wg_lgkm0, wg_pin), so no register copy of a
// read's destination can run before its data has landed.
template <int DT, bool RM>
struct WgRaw {
  using Piece = std::conditional_t<RM, s16x4, bf16x8>;
  static constexpr int NP = (IsSplit<DT>::value ? 2 : 1) * (RM ? 2 : 1);
  Piece p[NP];
};
// slot I of the quadrant at LDS address qb (uniform, or per lane half in the half-stage ring);
// FBS: bytes between slots; fmo / rmo: this lane's offsets (wgrad_lds_body)
template <int DT, bool RM, int FBS, int I>
DEV void wg_read(WgRaw<DT, RM>& r, unsigned qb, unsigned fmo, const unsigned (&rmo)[4][2]) {
  constexpr bool SP = IsSplit<DT>::value;
  if constexpr (RM) {
    constexpr int SUB = 4 * (SP ? 256 : 128);   // 4 image rows
    r.p[0] = tr4_at<0>(qb + rmo[I][0]);
    r.p[1] = tr4_at<SUB>(qb + rmo[I][0]);
    if constexpr (SP) {
      r.p[2] = tr4_at<0>(qb + rmo[I][1]);
      r.p[3] = tr4_at<SUB>(qb + rmo[I][1]);
    }
  } else {
    r.p[0] = lds_rd16_at<I * FBS>(qb + fmo);
    if constexpr (SP) r.p[1] = lds_rd16_at<I * FBS + 512>(qb + fmo);
  }
}
template <int DT, bool RM, int FBS>
DEV void wg_read4(WgRaw<DT, RM> (&r)[4], unsigned qb, unsigned fmo, const unsigned (&rmo)[4][2]) {
  wg_read<DT, RM, FBS, 0>(r[0], qb, fmo, rmo);
  wg_read<DT, RM, FBS, 1>(r[1], qb, fmo, rmo);
  wg_read<DT, RM, FBS, 2>(r[2], qb, fmo, rmo);
  wg_read<DT, RM, FBS, 3>(r[3], qb, fmo, rmo);
}
// every LDS read issued so far has landed: ONE s_waitcnt lgkmcnt(0) for the group, then each
// destination redefined by an (empty) asm statement — volatile asm statements keep their order, so
// no use of a destination is scheduled above the wait; the caller follows the group's pins with
// __builtin_amdgcn_sched_barrier(0) (register-only MFMAs are otherwise hoisted over an asm wait)
DEV void wg_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)"); }
template <int DT, bool RM>
DEV void wg_pin(WgRaw<DT, RM>& r) {
  if constexpr (WgRaw<DT, RM>::NP == 4) asm volatile("" : "+v"(r.p[0]), "+v"(r.p[1]), "+v"(r.p[2]), "+v"(r.p[3]));
  else if constexpr (WgRaw<DT, RM>::NP == 2) asm volatile("" : "+v"(r.p[0]), "+v"(r.p[1]));
  else asm volatile("" : "+v"(r.p[0]));
}
template <int DT, bool RM>
DEV typename Prec<DT>::Frag wg_frag(const WgRaw<DT, RM>& r) {
  if constexpr (IsSplit<DT>::value) {
    if constexpr (RM) return S3Frag{cat8(r.p[0], r.p[1]), cat8(r.p[2], r.p[3])};
    else return S3Frag{r.p[0], r.p[1]};
  } else {
    if constexpr (RM) return cat8(r.p[0], r.p[1]);
    else return r.p[0];
  }
}

// Tasks of up to 8 quadrants run one quadrant per wave (QW 1: 24 fragment slots per stage); split-bf16
// and bf16 tasks of 9-16 quadrants (nq even) run TWO per wave (QW 2: 40 slots, nq + kq <= 10), the
// wave's quadrants (wn, wk) and (wn + nq / 2, wk) sharing its X fragments — a wider tile streams fewer
// operand rows per output (Humanoid v_fc1 as four 4x3 quadrant tiles: 28 x 64 rows per k-step
// instead of 36 x 64 with six 4x2 tiles) and a wave reads 12 fragments per 32 MFMA tiles instead of
// 8 per 16.  The ring depth follows the stage size: split-bf16 3 stages of 24 slots or 2 of 40 (one
// stage in flight: a 4x3 tile's 3-stage ring would need 168 KiB; the wait share grows, 0.46 -> 0.52
// of the wave cycles, docs/ARCHITECTURE.md §13), bf16 4 of either.
//
// Split-bf16 wide tasks of <= 32 slots (C = 4: the 4x3 and 2x6 tiles) run a ring of HALF-stages
// instead (WgHalf): a 2 KiB split fragment is two 1 KiB DMA instructions, instruction h carrying
// rows 16 h .. 16 h + 15 of the k-step (the lanes 32 h .. 32 h + 31; of a row-major quadrant image
// its first / second 4 KiB), so a unit of 32 slots x 1 KiB holds half a step and 5 units fit the
// 160 KiB the 2 x 40-slot ring takes.  Step k reads units 2k and 2k + 1 (a lane reads the unit of
// its half, lane >> 5) and, past the barrier, refills the two units step k - 1 read with units
// 2k + 3 and 2k + 4, the older first, so the in-order vmcnt retires them in need order: the
// counted wait at the top of a step leaves unit 2k + 2 in flight across the barrier (the
// full-stage ring: nothing) and 1.5 steps are in flight after the refill (1).  Every wave issues
// 4 instructions per unit — it owns one quadrant's four slots: fragment-major, instruction h of
// each slot; row-major, the four 4-row instructions of the image's half h — so vmcnt(4) is
// exactly "all but the newest unit" on every wave.
#ifndef WGRAD_HALF_RING
#define WGRAD_HALF_RING 1   // 0: the full-stage ring for every wide task (A/B builds)
#endif
template <int DT, int QW>
struct WgCfg {
  static constexpr int SLOTS = QW == 1 ? 24 : 40;
  static constexpr int S = DT == DT_BF16 ? 4 : (QW == 1 ? 3 : 2);
};
struct WgHalf {
  static constexpr int SLOTS = 32, UNITS = 5, UB = SLOTS * 1024;   // bytes per unit
};
template <int DT, int QW, int C>
constexpr bool wgrad_half_ring() { return WGRAD_HALF_RING && DT == DT_S3 && QW == 2 && C == 4; }
template <int DT, bool WIDE>
constexpr size_t wgrad_lds_bytes() {
  constexpr size_t one = (size_t)WgCfg<DT, 1>::S * WgCfg<DT, 1>::SLOTS * wgrad_frag_bytes<DT>();
  constexpr size_t two = (size_t)WgCfg<DT, 2>::S * WgCfg<DT, 2>::SLOTS * wgrad_frag_bytes<DT>();
  constexpr size_t half = DT == DT_S3 ? (size_t)WgHalf::UNITS * WgHalf::UB : 0;
  constexpr size_t wide = two > half ? two : half;
  return WIDE && wide > one ? wide : one;
}
static_assert(wgrad_lds_bytes<DT_S3, true>() <= 160 * 1024 && wgrad_lds_bytes<DT_BF16, true>() <= 160 * 1024 &&
              wgrad_lds_bytes<DT_F32, false>() <= 160 * 1024 && wgrad_lds_bytes<DT_FP8, false>() <= 160 * 1024 &&
              (size_t)WgHalf::UNITS * WgHalf::UB <= 160 * 1024, "every wgrad ring fits the CU's 160 KiB of LDS");

// G_RM / X_RM: the dY / X operand of the task's layer is row-major (split-bf16 / bf16 only) — a
// property of the instantiation, chosen once per task at kernel entry (wgrad_by_layout): no layout
// branch inside the k-loop
template <int DT, int QW, int C, bool G_RM, bool X_RM>
DEV void wgrad_lds_body(const WgradArgs& a, const WgradTask& tk, char* smem) {
  using P = Prec<DT>;
  using T = typename P::T;
  using Frag = typename P::Frag;
  constexpr int FB = wgrad_frag_bytes<DT>();     // bytes per fragment
  constexpr int NI = FB / 1024;                  // DMA instructions per fragment (64 lanes x 16 B)
  constexpr int S = WgCfg<DT, QW>::S;
  constexpr int SB = WgCfg<DT, QW>::SLOTS * FB;  // bytes per stage
  constexpr bool RMOK = DT == DT_S3 || DT == DT_BF16;   // (fp32 / e4m3 operands are fragment-major only)
  constexpr bool HALF = wgrad_half_ring<DT, QW, C>();   // the ring of half-stage units (WgHalf)
  static_assert(QW == 1 || DT == DT_S3 || DT == DT_BF16, "two quadrants per wave: split-bf16 / bf16");
  static_assert(C * WG_WAVES <= WgCfg<DT, QW>::SLOTS, "slots");
  static_assert(RMOK || (!G_RM && !X_RM), "row-major operands: split-bf16 / bf16");
  static_assert(!HALF || (C * WG_WAVES == WgHalf::SLOTS && NI == 2), "half-stage ring: a quadrant per wave");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const char* g = reinterpret_cast<const char*>(a.gT[tk.layer]);
  const char* x = reinterpret_cast<const char*>(a.xT[tk.layer]);
  const int nk = (tk.m1 - tk.m0) / wgrad_step_rows<DT>();
  const int ks0 = tk.m0 >> 5;
  const int NF = 4 * tk.nq, F = NF + 4 * tk.kq;
  // slot f of a stage holds fragment f: f < NF -> dY^T row tile n0/16 + f, else X^T row tile
  // k0/16 + f - NF.  Wave w DMAs slots C*w .. C*w + C-1 (a slot >= F re-loads fragment f mod F).
  // FM operands: a fragment is contiguous (FB bytes per k-step).  Row-major operands (the 32x32
  // policy head's g1p / g2p / h1p and the observation rows, csrc/phead.hip; row length a.g_rm /
  // a.x_rm): a quadrant's 4 slots hold its [32 rows][64 features] image per k-step — bf16: 128-byte
  // rows, the 16-byte chunks XOR-swizzled by wgrad_swz(row), 8 rows per DMA instruction;
  // split-bf16: the memory's 256-byte [8 hi | 8 lo] rows, wgrad_swz16, 4 rows per instruction —
  // read back transposed (ds_read_b64_tr_b16).
  const char* srcp[C][NI];
  size_t kstride[C];
  int dst[C];
#pragma unroll
  for (int q = 0; q < C; ++q) {
    const int f = wave * C + q;
    const int ff = f < F ? f : f % F;   // dummy slot: re-load one of the task's fragments
    const bool gs = ff < NF;
    const int fl = gs ? ff : ff - NF;
    const int feat0 = (gs ? tk.n0 : tk.k0) + 16 * fl;
    // rm: 0 fragment-major; > 0 row-major rows of rm elements
    const int rm = gs ? (G_RM ? a.g_rm[tk.layer] : 0) : (X_RM ? a.x_rm[tk.layer] : 0);
    const char* ob = gs ? g : x;
    if (rm == 0) {
      const char* src = ob + fm_frag(feat0 >> 4, ks0, a.ld, 0) * sizeof(T);
#pragma unroll
      for (int hh = 0; hh < NI; ++hh)
        srcp[q][hh] = src + (IsSplit<DT>::value ? (size_t)hh * 1024 + (lane & 31) * 32 + (lane >> 5) * 16
                                                 : (size_t)hh * 1024 + lane * 16);
      kstride[q] = FB;
    } else {
      const int sq = fl & 3, f0 = feat0 - 16 * sq;   // slot in the quadrant, the quadrant's first feature
#pragma unroll
      for (int hh = 0; hh < NI; ++hh) {
        const int n = NI * sq + hh;                   // 1 KiB DMA instruction of the quadrant image
        if constexpr (IsSplit<DT>::value) {           // rows 4 n .. 4 n + 3, 256 bytes each
          const int row = 4 * n + (lane >> 4);
          const int c = (lane & 15) ^ wgrad_swz16(row);
          srcp[q][hh] = ob + ((size_t)(tk.m0 + row) * rm + f0) * sizeof(T) + 16 * c;
        } else {                                      // rows 8 n .. 8 n + 7, 128 bytes each
          const int row = 8 * n + (lane >> 3);
          const int c = (lane & 7) ^ wgrad_swz(row);
          srcp[q][hh] = ob + ((size_t)(tk.m0 + row) * rm + f0 + 8 * c) * sizeof(T);
        }
      }
      kstride[q] = (size_t)32 * rm * sizeof(T);
    }
    dst[q] = f * FB;
  }
  // a full stage: step k's C slots of this wave into stage k mod S
  auto issue = [&](int k) {
    const int kk = min(k, nk - 1);            // past the end: re-load valid data (count stays fixed)
    char* st = smem + (k % S) * SB;
#pragma unroll
    for (int q = 0; q < C; ++q)
#pragma unroll
      for (int h = 0; h < NI; ++h) glds16(srcp[q][h] + (size_t)kk * kstride[q], st + dst[q] + h * 1024);
  };
  // the half-stage ring: this wave's 4 instructions of half H of step k, in unit order (its quadrant
  // fragment-major: instruction H of each of its slots; row-major: instructions 4 H .. 4 H + 3 of the
  // image, which are slots 2 H, 2 H + 1), into the unit at ring position pos — slot 4 wave + j at
  // j KiB of the wave's 4 KiB of the unit either way
  const char* usrc[2][4];
  if constexpr (HALF) {
    const bool rmw = (wave * C < F ? wave * C : (wave * C) % F) < NF ? G_RM : X_RM;   // (wave-uniform)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 4; ++j) usrc[h][j] = rmw ? srcp[2 * h + (j >> 1)][j & 1] : srcp[j][h];
  }
  auto issue_half = [&](auto H, int k, int pos) __attribute__((always_inline)) {
    const int kk = min(k, nk - 1);
    char* ub = smem + pos * WgHalf::UB + wave * 4096;
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(usrc[H.value][j] + (size_t)kk * kstride[0], ub + j * 1024);
  };
  auto mod5 = [](int u) { return u >= WgHalf::UNITS ? u - WgHalf::UNITS : u; };
  // Q8: this lane's sub-slot maximum of the layer's gradient tensor, loaded before any DMA (the
  // oldest vector-memory op: it never holds up a counted wait), folded in the epilogue
  uint32_t q8v = 0;
  if constexpr (DT == DT_FP8) q8v = a.q8_rd[(a.q8_t[tk.layer] * Q8_SUB + lane) * Q8_LINE];
  // QW 2: waves (wn, wk) for wn < nq / 2, quadrant rows wn and wn + nq / 2
  const int nqw = QW == 1 ? tk.nq : tk.nq >> 1;
  const bool active = wave < nqw * tk.kq;
  const int wn = wave / tk.kq, wk = wave - (wave / tk.kq) * tk.kq;
  // per-lane byte offsets within a quadrant's 4 slots: fragment-major, the lane's 16 bytes of slot i
  // at fmo + i * FBS (FBS: bytes between slots; a half-stage unit holds 1 KiB of each, its lanes'
  // [hi][lo]); row-major, the first 4-row transposed read of slot i (split: of its hi, lo part) —
  // the same pattern for every quadrant and side (a quadrant adds its slot base)
  constexpr int FBS = HALF ? 1024 : FB;
  const unsigned fmo = HALF ? (unsigned)((lane & 31) * 16)
                            : IsSplit<DT>::value ? (unsigned)((lane >> 5) * 1024 + (lane & 31) * 16)
                                                 : (unsigned)(lane * 8 * (int)sizeof(T));
  unsigned rmo[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rmo[i][0] = rmo[i][1] = 0;
    if constexpr (IsSplit<DT>::value) {
      rmo[i][0] = rm_off_s3(i, 0, 0, lane, FB, HALF ? 15 : 31);
      rmo[i][1] = rm_off_s3(i, 0, 1, lane, FB, HALF ? 15 : 31);
    } else if constexpr (RMOK) {
      rmo[i][0] = rm_off(i, 0, lane, FB);
    }
  }
  const unsigned lds0 = lds_addr(smem);
  f32x4 acc[QW][4][4];
#pragma unroll
  for (int u = 0; u < QW; ++u)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[u][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int p5 = 0;   // half-stage ring: the ring position of unit 2k
  if constexpr (HALF) {
    issue_half(std::integral_constant<int, 0>{}, 0, 0);
    issue_half(std::integral_constant<int, 1>{}, 0, 1);
    issue_half(std::integral_constant<int, 0>{}, 1, 2);
  } else {
#pragma unroll
    for (int s = 0; s < S - 1; ++s) issue(s);
  }
  for (int k = 0; k < nk; ++k) {
    // this wave's part of stage k has landed (half-stage ring: of units 2k, 2k + 1; unit 2k + 2
    // stays in flight)
    if constexpr (HALF) WAIT_VMCNT(4);
    else WAIT_VMCNT(C * NI * (S - 2));
    __builtin_amdgcn_s_barrier();              // ... everyone's; and stage k-1 is no longer read
    // refill the slot stage k-1 used: split-bf16 / bf16 after this step's fragment reads are
    // issued (the DMA issue cost then overlaps their latency: 4.16 vs 4.22 ms per bf16x3 iteration,
    // 2.30 vs 2.32 bf16, same box); e4m3 right here (2.01 vs 1.99 the other way;
    // profiles/r4/ab_late_issue_*.json)
    constexpr bool LATE = DT != DT_FP8;
    auto refill = [&]() __attribute__((always_inline)) {
      if constexpr (HALF) {   // units 2k + 3, 2k + 4 into the places of 2k - 2, 2k - 1
        issue_half(std::integral_constant<int, 1>{}, k + 1, mod5(p5 + 3));
        issue_half(std::integral_constant<int, 0>{}, k + 2, mod5(p5 + 4));
      } else {
        issue(k + S - 1);
      }
    };
    if (!LATE || !active) refill();
    if (active) {
      if constexpr (DT == DT_FP8) {
        static_assert(DT != DT_FP8 || QW == 1, "the e4m3 scale epilogue covers acc[0] only");
        const char* st = smem + (k % S) * SB;
        // four e4m3 k-steps per slot: lane l's 8 bytes of k-step 4kk + j at j * 512 + l * 8.  The
        // 16x16x128 operand of lane l is those 32 bytes in j order — rows {32 j + 8 (l >> 4) + e}
        // for BOTH operands, so the MFMA's k sum runs over every row of the 128 exactly once
        // (E8M0 scales 127 = 1: the power-of-two operand scales are undone in the epilogue)
        auto rd = [&](int f) {
          const char* p = st + f * FB + lane * 8;
          const long x0 = *reinterpret_cast<const long*>(p), x1 = *reinterpret_cast<const long*>(p + 512);
          const long x2 = *reinterpret_cast<const long*>(p + 1024), x3 = *reinterpret_cast<const long*>(p + 1536);
          return i32x8{(int)x0, (int)(x0 >> 32), (int)x1, (int)(x1 >> 32), (int)x2, (int)(x2 >> 32), (int)x3,
                       (int)(x3 >> 32)};
        };
        i32x8 a8[4], b8[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a8[i] = rd(wn * 4 + i);
          b8[i] = rd(NF + wk * 4 + i);
        }

#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[0][i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8[i], b8[j], acc[0][i][j], 0, 0, 0, 127, 0, 127);
        continue;
      } else if constexpr (!RMOK) {   // fp32: plain LDS loads of the fragment-major slots
        const char* st = smem + (k % S) * SB;
        Frag af[4], bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          af[i] = P::load(reinterpret_cast<const T*>(st + (4 * wn + i) * FB + fmo));
          bf[i] = P::load(reinterpret_cast<const T*>(st + (NF + 4 * wk + i) * FB + fmo));
        }
        issue(k + S - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[0][i][j] = P::mma(acc[0][i][j], af[i], bf[j]);
      } else {
        // the stage's LDS address: uniform, or in the half-stage ring that of this lane half's unit
        unsigned sa;
        if constexpr (HALF) sa = lds0 + (unsigned)((lane >> 5) ? mod5(p5 + 1) : p5) * WgHalf::UB;
        else sa = lds0 + (unsigned)((k % S) * SB);
        // the step's first read group — the 8 fragments of the wave's (first) quadrant — issued
        // back to back, the refill's DMA instructions behind them, then one settle
        WgRaw<DT, G_RM> ar[4];
        WgRaw<DT, X_RM> br[4];
        wg_read4<DT, G_RM, FBS>(ar, sa + 4 * wn * FBS, fmo, rmo);
        wg_read4<DT, X_RM, FBS>(br, sa + (NF + 4 * wk) * FBS, fmo, rmo);
        refill();
        wg_lgkm0();
#pragma unroll
        for (int i = 0; i < 4; ++i) wg_pin(ar[i]);
#pragma unroll
        for (int i = 0; i < 4; ++i) wg_pin(br[i]);
        __builtin_amdgcn_sched_barrier(0);
        Frag af[4], bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          af[i] = wg_frag(ar[i]);
          bf[i] = wg_frag(br[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[0][i][j] = P::mma(acc[0][i][j], af[i], bf[j]);
        if constexpr (QW == 2) {
          // the second quadrant's dY fragments (its X fragments are the first's): the second
          // read group, one settle
          wg_read4<DT, G_RM, FBS>(ar, sa + 4 * (wn + nqw) * FBS, fmo, rmo);
          wg_lgkm0();
#pragma unroll
          for (int i = 0; i < 4; ++i) wg_pin(ar[i]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 4; ++i) af[i] = wg_frag(ar[i]);
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[QW - 1][i][j] = P::mma(acc[QW - 1][i][j], af[i], bf[j]);
        }
      }
    }
    if constexpr (HALF) p5 = mod5(p5 + 2);
  }
  WAIT_VMCNT(0);                               // no DMA may outlive the workgroup's LDS
  if (!active) return;
  const int KE = tk.kq * 64;
  float* out = a.slab + tk.slab;
  if constexpr (DT == DT_FP8) {   // undo the operands' scales (powers of two: exact)
    const float inv = q8_pow2(-q8_exp(wave_umax(q8v))) / a.q8_xs[tk.layer];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[0][i][j] *= inv;
  }
  const int col = wk * 64 + (lane & 15);
#pragma unroll
  for (int u = 0; u < QW; ++u) {
    const int rbase = (wn + u * nqw) * 64 + (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) out[(rbase + 16 * i + q) * KE + col + 16 * j] = acc[u][i][j][q];
  }
}

// the loop body of the task's operand layouts (a wave-uniform dispatch, like QW / C): p_fc1 is
// row-major / row-major, v_fc1 over x_buf's rows fragment-major / row-major, v_fc2 fragment-major
// both, p_fc1 over a fragment-major x^T row-major / fragment-major
template <int DT, int QW, int C>
DEV void wgrad_by_layout(const WgradArgs& a, const WgradTask& tk, char* smem) {
  if constexpr (DT == DT_S3 || DT == DT_BF16) {
    const bool g_rm = a.g_rm[tk.layer] != 0, x_rm = a.x_rm[tk.layer] != 0;
    if (g_rm) {
      if (x_rm) wgrad_lds_body<DT, QW, C, true, true>(a, tk, smem);
      else wgrad_lds_body<DT, QW, C, true, false>(a, tk, smem);
    } else {
      if (x_rm) wgrad_lds_body<DT, QW, C, false, true>(a, tk, smem);
      else wgrad_lds_body<DT, QW, C, false, false>(a, tk, smem);
    }
  } else {
    wgrad_lds_body<DT, QW, C, false, false>(a, tk, smem);
  }
}

// WIDE: the launch holds two-quadrant-per-wave tasks (wgrad_task_ok), the LDS of either ring
template <int DT, bool WIDE>
__global__ __launch_bounds__(WG_WAVES * 64) void wgrad_kernel(WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // the kernel's ONLY LDS object
  const WgradTask tk = a.tasks[blockIdx.x];
  const int F = 4 * (tk.nq + tk.kq);
  if constexpr (WIDE) {
    if (tk.nq * tk.kq > WG_WAVES) {
      if (F <= 4 * WG_WAVES) wgrad_by_layout<DT, 2, 4>(a, tk, smem);
      else wgrad_by_layout<DT, 2, 5>(a, tk, smem);
      return;
    }
  }
  if (F <= 2 * WG_WAVES) wgrad_by_layout<DT, 1, 2>(a, tk, smem);
  else wgrad_by_layout<DT, 1, 3>(a, tk, smem);
}

template <int DT, bool WIDE>
void launch_wgrad_lds(const WgradArgs& a, hipStream_t s) {
  const size_t lds = wgrad_lds_bytes<DT, WIDE>();
  set_max_lds_once<wgrad_kernel<DT, WIDE>>(lds);
  hipLaunchKernelGGL((wgrad_kernel<DT, WIDE>), dim3(a.ntasks), dim3(WG_WAVES * 64), lds, s, a);
}

// Blocks [0, item_blocks(nitems)): the reduce items (log_std, loss-term sums, the per-head
// kernels' fused narrow-layer weight gradients): column sums of the per-workgroup partial rows in
// a fixed order (item_reduce), grad[d] = scale * sum or loss_out[q] (red_dst).
// Blocks past them: grad[i] = scale * sum_{c < nch} slab[src_off[i] + c * stride] for the slab
// elements i of `runs` (src_meta[i] = nch * 32 + stride / 4096, each tile has its own batch-chunk
// count).  Fixed chunk order: deterministic; no float atomics anywhere.
// STREAM: the same sums over the quads of the tile table (kernels.h SlabTiles, common.h slab_sum4).
template <bool STREAM>
__global__ __launch_bounds__(256) void grad_gather_kernel(const float* __restrict__ slab,
                                                          const int* __restrict__ src_off,
                                                          const int* __restrict__ src_meta,
                                                          const float* __restrict__ part,
                                                          int nblk, int npart, const int* __restrict__ red_col,
                                                          const int* __restrict__ red_dst, int nitems,
                                                          float scale, float* __restrict__ grad, SlabRuns runs,
                                                          float* __restrict__ loss_out, SlabTiles tiles) {
  const int nrb = item_blocks(nitems);
  if ((int)blockIdx.x < nrb) {
    __shared__ float red[256];
    float tot = 0.f;
    int j;
    if (item_reduce(part, nblk, npart, red_col, nitems, blockIdx.x, red, tot, j)) {
      const int d = red_dst[j];
      if (d >= 0) grad[d] = tot * scale;
      else loss_out[-1 - d] = tot;
    }
    return;
  }
  const int nb = gridDim.x - nrb;
  if constexpr (STREAM) {
    __shared__ int tl[SLAB_TILES_MAX * SLAB_TILE_INTS];
    slab_tiles_stage(tiles, tl);
    for (int Q = (blockIdx.x - nrb) * 256 + threadIdx.x; Q < tiles.nquads; Q += nb * 256) {
      const SlabQuad q = slab_quad(tl, tiles.n, Q, slab);
      const float4 s = slab_sum4(q.src, q.nch, q.st4);
      const float sl[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (q.i[l] >= 0) grad[q.i[l]] = sl[l] * scale;
    }
  } else {
    for (int j = (blockIdx.x - nrb) * 256 + threadIdx.x; j < runs.total; j += nb * 256) {
      const int i = runs.flat(j);
      const int mt = src_meta[i];
      const int o = src_off[i];
      const int nch = mt >> 5;
      const size_t st = (size_t)(mt & 31) << 12;
      const float s = slab_sum(slab + o, nch, st);
      grad[i] = s * scale;
    }
  }
}

}  // namespace

// a task's quadrant tile: one quadrant per wave (nq * kq <= 8, nq + kq <= 6: 24 slots), or at
// split-bf16 / bf16 two per wave (9-16 quadrants, nq even, nq + kq <= 10: 40 slots)
extern "C" int wgrad_task_ok(int dt, int nq, int kq) {
  if (nq < 1 || kq < 1) return 0;
  if (nq * kq <= WG_WAVES) return nq + kq <= 6;
  return (dt == DT_S3 || dt == DT_BF16) && nq * kq <= 2 * WG_WAVES && nq % 2 == 0 && nq + kq <= 10;
}

extern "C" void launch_wgrad(int dt, const WgradArgs& a, hipStream_t s) {
  if (a.ntasks <= 0) return;
  if (dt == DT_F32) launch_wgrad_lds<DT_F32, false>(a, s);
  else if (dt == DT_FP8) launch_wgrad_lds<DT_FP8, false>(a, s);
  else if (dt == DT_S3) {
    if (a.wide) launch_wgrad_lds<DT_S3, true>(a, s);
    else launch_wgrad_lds<DT_S3, false>(a, s);
  } else {
    if (a.wide) launch_wgrad_lds<DT_BF16, true>(a, s);
    else launch_wgrad_lds<DT_BF16, false>(a, s);
  }
  HIP_CHECK_LAUNCH();
}

extern "C" void launch_grad_gather(const GatherArgs& ga, float* grad, hipStream_t s) {
  const bool stream = ga.tiles.t != nullptr && gather_stream_on();
  int grid = ((stream ? ga.tiles.nquads : ga.runs.total) + 255) / 256;   // one quad / element per thread
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  grid += item_blocks(ga.nitems);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, ga.slab, ga.src_off, ga.src_meta, ga.part, ga.npblk,
                       ga.npart, ga.red_col, ga.red_dst, ga.nitems, ga.scale, grad, ga.runs, ga.loss_out, ga.tiles);
  };
  if (stream) go(grad_gather_kernel<true>);
  else go(grad_gather_kernel<false>);
  HIP_CHECK_LAUNCH();
}
