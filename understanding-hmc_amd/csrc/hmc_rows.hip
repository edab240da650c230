// hmc_rows.hip — four chains per wavefront for the FAST identity-target Random kernel, D = 97..112.
//
// Same semantics and the same per-coordinate arithmetic as the production wave-per-chain instance
// (hmc_wave.hip: FAST, identity precision and mass, Philox, three-term leapfrog, no capture), in
// another layout: chain 4 * wave + r lives in the 16-lane DPP row r, and lane s of the row holds
// coordinates s + 16 j, j < 7 (slots past D hold exact zeros).  What the wave kernel pays once per
// wave (the energy reduction, the accept test, parking, tallies, addresses) is paid once per four
// chains here.  Every q is bit-identical to the wave kernel's; the energies are row sums (one
// chain for both: a fold by eight lanes, then row_shr 1/2/4) instead of the full-wave sum, so E and
// dE move in the last bits.
//   * trajectory lengths differ per row: the paired-step loop runs to the wave's longest
//     trajectory (known since the 16-iteration draw of L) and rows that are done are switched off
//     through EXEC;
//   * the energy lands in lane 15 of each row and the decision is formed in lane 7; its four bits
//     are widened to row masks on the SALU, and a reject restores under that EXEC mask;
//   * the state lives in one of two register sets and the trajectory is integrated into the other, so
//     the set it started from is the restore point and nothing is copied per iteration; the next
//     iteration swaps the two roles (the loop body stands twice per trip, role as a template constant);
//   * momentum: every pass draws 16 consecutive pairs of each row's own (pair, iteration) stream
//     into that chain's LDS ring (stream order, ten 128-B chunks; the first is mirrored behind the
//     tenth, so that a read which starts in the last chunk runs on without a per-lane wrap).  The
//     Philox block starts from a per-block table of what rounds 1-2 derive from the pair alone
//     (hmc_philox_split.hpp); -DHMC_ROWS_NO_SPLIT keeps the whole block, for an A/B of the table.
// Odd D needs no instance of its own: coordinates are read from the ring one by one, so the pair
// that holds the dimension past D is only ever read by a masked slot.
// Dynamic LDS: the Box–Muller tables (32 KB) + the split-Philox table of the block's pairs (1 KB) +
// 8 waves x 4 chains x 1408 B = 77 KB per block: two blocks per CU (154 of its 160 KB), four waves per
// SIMD (no scratch).  Two blocks rather than one of 16 waves: a block's start-up (tables, state loads,
// first ring fill) and its tail then overlap the other's iterations (measured 5% faster).
// The kernel has no static LDS, so the dynamic allocation starts at LDS byte 0 (the launcher checks
// it): every LDS address is formed as a 32-bit byte offset with the region's start as a constant,
// which lands in the instruction's immediate offset instead of an add of the allocation's base.
#include "hmc_device.hpp"
#include "hmc_philox_split.hpp"
#include "hmc_internal.hpp"
#include "hmc_target_ops.hpp"

namespace hmc {

namespace {

constexpr int kRowLanes = 16;                      // one DPP row per chain
constexpr int kRowChains = kWave / kRowLanes;      // chains per wave
constexpr int kRowsBlock = 512;                    // 8 waves
constexpr int kRowChunkBytes = 8 * kRowLanes;      // one slot of a row: 16 doubles
constexpr uint32_t kRowRingBytes = 10 * kRowChunkBytes;   // per chain: at most (112 - 1) + 32 doubles wait in it
constexpr uint32_t kRowRingAlloc = 11 * kRowChunkBytes;   // + the mirror of chunk 0 (reads end 248 B past a chunk's start)
constexpr int kRowMaxPairs = 56;                   // D <= 112
constexpr uint32_t kRowSplitOff = 8 * kNormalTableDoubles;             // split-Philox table: behind the Box–Muller tables
constexpr uint32_t kRowRingOff = kRowSplitOff + 1024;                  // 56 entries x 16 B, padded to 1 KB
constexpr size_t kRowsLds = kRowRingOff + (size_t)(kRowsBlock / kWave) * kRowChains * kRowRingAlloc;
static_assert(16 * kRowMaxPairs <= 1024 && kRowRingOff + kRowRingBytes + 16 * kRowLanes < 65536,
              "the table fits its region and every region start fits the 16-bit immediate offset");
static_assert(2 * kRowsLds <= 160 * 1024, "two blocks per CU");

// LDS byte offset -> pointer (the offset is a run-time value for the language: no null constant)
template <class T>
__device__ __forceinline__ __attribute__((address_space(3))) T* lds_at(uint32_t off) {
  return (__attribute__((address_space(3))) T*)(uintptr_t)off;
}
typedef uint32_t lds_u32x4 __attribute__((ext_vector_type(4)));
typedef double lds_f64x2 __attribute__((ext_vector_type(2)));

// x.x of the lane's coordinates, the chain hmc_wave.hip's wave_sumsq_fma forms
template <int C>
__device__ __forceinline__ double rows_sumsq(const double (&v)[C], double s0) {
  double s = __builtin_fma(v[1], v[1], s0);
  s = __builtin_fma(v[0], v[0], s);
#pragma unroll
  for (int e = 2; e < C; ++e) s = __builtin_fma(v[e], v[e], s);
  return s;
}

// DPP move of src into the lanes of the banks in BANK_MASK (four lanes each); the other lanes keep old
template <int CTRL, int BANK_MASK>
__device__ __forceinline__ double dpp_banks(double old, double src) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, 0xF, BANK_MASK, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, 0xF, BANK_MASK, false);
  return __hiloint2double(hi, lo);
}

// Two sums over each 16-lane row in one chain (EXEC all ones): both are first folded by eight lanes
// into one register, lo into lanes 0-7 (lo[i] + lo[i + 8]) and hi into lanes 8-15 (hi[i - 8] + hi[i]),
// then row_shr 1/2/4 finish both at once: lane 7 of the row holds the total of lo, lane 15 that of hi.
__device__ __forceinline__ double row_sum2_l7_l15(double lo, double hi) {
  double o = __hiloint2double(__builtin_amdgcn_mov_dpp(__double2hiint(lo), 0x108, 0xF, 0x3, false),
                              __builtin_amdgcn_mov_dpp(__double2loint(lo), 0x108, 0xF, 0x3, false));   // row_shl:8 -> lanes 0-7
  o = dpp_banks<0x118, 0xC>(o, hi);                   // row_shr:8 -> lanes 8-15
  double v = dpp_banks<0xE4, 0xC>(lo, hi);            // quad_perm:[0,1,2,3]: hi as it is in lanes 8-15
  v += o;
  v += dpp_u<0x111>(v);        // row_shr:1 (bound_ctrl: lanes shifted in from outside the row read 0)
  v += dpp_u<0x112>(v);        // row_shr:2
  v += dpp_u<0x114>(v);        // row_shr:4
  return v;
}

// sum over each 16-lane row of per-lane integer tallies: lane 15 of the row holds the total
__device__ __forceinline__ uint32_t row_sum_u32_l15(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);
  return v;
}

// n += 1 in the lanes of `mask` (one VALU: the mask is the carry-in)
__device__ __forceinline__ void add_mask(uint32_t& n, uint64_t mask) {
  uint64_t co;
  asm("v_addc_co_u32_e64 %0, %1, %0, 0, %2" : "+v"(n), "=&s"(co) : "s"(mask));
}

constexpr uint64_t kRowLane15 = 0x8000800080008000ull;   // lane 15 of every row
constexpr uint64_t kRowLane7 = 0x0080008000800080ull;    // lane 7 of every row

// Parks e in Ebuf and d in dEbuf (both valid in lane 15 of each row): each row of a buffer moves one
// lane down and takes the value in lane 15, so after n parks the values sit in lanes 16 - n .. 15,
// oldest first.  No LDS round trip.  One select per word, in place: the DPP operand is the buffer
// shifted by row_shl:1 (lane 15 has no source and reads 0 under bound_ctrl), the select mask (VCC)
// is lane 15 of every row, where the value is taken instead.  The buffers were last written by the
// park before, so no DPP read follows a write of its register within the hazard's two wait states.
__device__ __forceinline__ void park_rows(double& Ebuf, double& dEbuf, double e, double d, uint64_t lane15) {
  int el = __double2loint(Ebuf), eh = __double2hiint(Ebuf), dl = __double2loint(dEbuf), dh = __double2hiint(dEbuf);
  asm("s_mov_b64 vcc, %[m]\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_dpp %[el], %[el], %[vel], vcc row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_cndmask_b32_dpp %[eh], %[eh], %[veh], vcc row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_cndmask_b32_dpp %[dl], %[dl], %[vdl], vcc row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_cndmask_b32_dpp %[dh], %[dh], %[vdh], vcc row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
      : [el] "+v"(el), [eh] "+v"(eh), [dl] "+v"(dl), [dh] "+v"(dh)
      : [vel] "v"(__double2loint(e)), [veh] "v"(__double2hiint(e)), [vdl] "v"(__double2loint(d)),
        [vdh] "v"(__double2hiint(d)), [m] "s"(lane15)
      : "vcc");
  Ebuf = __hiloint2double(eh, el);
  dEbuf = __hiloint2double(dh, dl);
}

template <int C>
__global__ __launch_bounds__(kRowsBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_rows_iters(RandArgs a) {
  static_assert(C == 7, "seven coordinates per lane: D in (96, 112], only the last slot is partial");
  const double* const s_ntab = (const double*)lds_at<double>(0);   // Box–Muller tables
  init_normal_tables((double*)lds_at<double>(0));
  // The split-Philox table of this block: entry k of pair k under the seed's high word and the high
  // word of the block's first chain id.
  constexpr int chains_per_block = (kRowsBlock / kWave) * kRowChains;
  const uint32_t tab_ghi = (uint32_t)((uint64_t)(a.chain_offset + (int64_t)blockIdx.x * chains_per_block) >> 32);
  if ((int)threadIdx.x < a.npairs) {
    const uint4 e = split_entry(threadIdx.x, tab_ghi, a.k1);
    *lds_at<lds_u32x4>(kRowSplitOff + 16u * threadIdx.x) = lds_u32x4{e.x, e.y, e.z, e.w};
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = threadIdx.x / kWave;
  const int64_t c0 = (int64_t)kRowChains * uniform_i(blockIdx.x * (kRowsBlock / kWave) + wib);
  if (c0 >= a.n) return;                                  // whole wave, uniform
  const int r = lane / kRowLanes, s = lane & (kRowLanes - 1);
  const int64_t c = c0 + r;
  const bool valid = c < a.n;                             // rows past the last chain run along; masked at loads, stores, tallies
  const bool v6 = s + kRowLanes * (C - 1) < a.D;          // the last slot exists for this lane
  const bool st6 = valid && v6;
  const uint64_t gc = (uint64_t)(a.chain_offset + c);
  const uint32_t ringrow = (uint32_t)(wib * kRowChains + r) * kRowRingAlloc;   // this chain's ring (bytes)
  // The table serves a wave whose valid rows all have its high word (rows past the last chain are
  // never stored: they may draw another chain's stream).  A wave with a row across a 2^32 boundary of
  // the global chain id draws with draw_block instead; decided here once, uniform.
#ifdef HMC_ROWS_NO_SPLIT
  const bool split = false;
#else
  const bool split = __builtin_amdgcn_ballot_w64(valid && (uint32_t)(gc >> 32) != tab_ghi) == 0;
#endif
  uint32_t sp_a, sp_b;                                    // the lane's loop-invariant words of rounds 1-2
  split_lane_words((uint32_t)gc, a.k0, sp_a, sp_b);

  // Generator: lane s of a row draws pair gkb / 16 of iteration git of its chain; a pass moves it 16
  // pairs on (npairs >= 49: one wrap at most).  The pair index is kept in bytes of the split table.
  // gen_n: pairs drawn per chain, gposb: their ring position.
  int gen_n = 0;
  uint32_t gposb = 0;
  uint32_t gkb = 16 * s, git = a.it0;
  const uint32_t wlane = ringrow + 16 * s;
  int rbaseb = 0;                                         // ring position (bytes) of the next iteration's doubles
  const int dpb = 16 * a.npairs;                          // stream bytes per iteration
  const uint32_t rlane = ringrow + 8 * s;
  double q[C], qt[C], p[C];                             // the two state sets (roles swap per iteration) and the momentum
  // 16 pairs on: gkb += 256, and past the iteration's last pair gkb -= 16 npairs, git += 1 (four VALU:
  // the borrow of gkb - 16 npairs picks both)
  auto advance = [&](uint32_t& k, uint32_t& i) {
    uint64_t bo;
    uint32_t tk;
    asm("v_add_u32_e32 %0, 0x100, %0\n\t"
        "v_subrev_co_u32_e32 %2, vcc, %4, %0\n\t"
        "v_subb_co_u32_e64 %1, %3, %1, -1, vcc\n\t"
        "v_cndmask_b32_e32 %0, %2, %0, vcc"
        : "+v"(k), "+v"(i), "=&v"(tk), "=&s"(bo)
        : "s"(dpb)
        : "vcc");
  };
  auto ring_momentum = [&](int it) {
    const int need = (it - a.it0 + 1) * a.npairs;
    while (gen_n < need) {                                // wave-uniform
      double z0, z1;
      uint4 blk;
      if (split) {
        const lds_u32x4 e = *lds_at<lds_u32x4>(kRowSplitOff + gkb);
        blk = split_block(make_uint4(e.x, e.y, e.z, e.w), sp_a, sp_b, git, a.k0, a.k1);
      } else {
        blk = draw_block(gkb >> 4, git, gc, a.k0, a.k1);
      }
      normal_pair_tab(blk, s_ntab, z0, z1);
      // a pass fills two whole chunks (1280 = 5 * 256: it never straddles the wrap)
      const uint32_t w = gposb + wlane;
      *lds_at<lds_f64x2>(kRowRingOff + w) = lds_f64x2{z0, z1};
      // the mirror of chunk 0: the pass's first eight pairs
      if (gposb == 0 && s < kRowLanes / 2) *lds_at<lds_f64x2>(kRowRingOff + kRowRingBytes + w) = lds_f64x2{z0, z1};
      gen_n += kRowLanes;
      gposb += 16 * kRowLanes;
      if (gposb >= kRowRingBytes) gposb -= kRowRingBytes;
      advance(gkb, git);
    }
    __builtin_amdgcn_wave_barrier();
    // slot j starts in chunk (cb + j) mod 10 (SALU) and this lane reads ob + 8 s bytes on, possibly
    // in the next chunk (the mirror after the tenth)
    const uint32_t cbb = (uint32_t)rbaseb & ~(uint32_t)(kRowChunkBytes - 1);
    const uint32_t a0 = ((uint32_t)rbaseb - cbb) + rlane;   // < 128 + 120
#pragma unroll
    for (int j = 0; j < C; ++j) {
      uint32_t cj = cbb + kRowChunkBytes * j;
      if (cj >= kRowRingBytes) cj -= kRowRingBytes;
      // The last slot is read under EXEC by the lanes that own a coordinate in it.  The others keep the
      // zero the slot was given before the loop: a zero coordinate with a zero momentum stays an exact
      // zero through every leapfrog step (p's registers hold x between two draws), so no select follows
      // the read.  (st6, not v6: what a row past the last chain holds there is never stored, and one
      // mask less stays in SGPRs through the loop.)
      if (j < C - 1 || st6) p[j] = *lds_at<double>(kRowRingOff + (opaque_s32(cj) + a0));
    }
    rbaseb += dpb;
    if (rbaseb >= (int)kRowRingBytes) rbaseb -= kRowRingBytes;
  };

  // the state: wave-uniform base (chain c0) + this lane's 32-bit byte offset, as every address below
  // (a 64-bit address per lane kept to the end of the kernel costs two VGPRs each)
  char* const qstb = reinterpret_cast<char*>(a.q + c0 * (int64_t)a.D);
  const uint32_t qstoff = (uint32_t)(r * a.D + s) * 8u;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    q[j] = 0.0;
    if (j < C - 1 ? valid : st6) q[j] = reinterpret_cast<const double*>(qstb + qstoff)[kRowLanes * j];
  }
  double Eprev = valid ? reinterpret_cast<const double*>(reinterpret_cast<char*>(a.Eprev + c0) + 8u * r)[0] : 0.0;
  __builtin_amdgcn_s_waitcnt(0x0F70);                    // retire state loads before the loop (vmcnt(0))

  p[C - 1] = 0.0;                                        // dimension past D: no such coordinate
  ring_momentum(a.it0);
  const double hlogc = 0.5 * a.logc;
  const uint64_t lane15 = kRowLane15;
  double ml = rows_sumsq<C>(q, 0.0), mtl = 0.0;          // this lane's part of q.q, of either state set
  double e0l = rows_sumsq<C>(p, ml);                     // ... and of q.q + p.p at the iteration start
  double Et = 0.0;                                       // the energy of an iteration: Eprev and Et swap roles too

  int row = 0, phase = 0;
  if (a.it0 >= a.wu) {
    row = (a.it0 - a.wu) / a.thin;
    phase = (a.it0 - a.wu) - row * a.thin;
  }
  int qslot = row % a.Lq;
  double Ebuf = 0.0, dEbuf = 0.0;
  int row_first = 0, nbuf = 0;
  const uint32_t bprow = (uint32_t)(lane & ~(kRowLanes - 1)) * 4;
  char* const Ecb = a.Ec ? reinterpret_cast<char*>(a.Ec + c0 * (int64_t)a.Lc) : nullptr;
  char* const dEcb = a.dEc ? reinterpret_cast<char*>(a.dEc + c0 * (int64_t)a.Lc) : nullptr;
  const uint32_t eoff = (uint32_t)(r * a.Lc + s) * 8u;         // host: 3 Lc 8 + 128 < 2^31
  // sample rows: wave-uniform base (chain c0, row qslot) + this lane's 32-bit byte offset
  char* const qcb = a.qc ? reinterpret_cast<char*>(a.qc + c0 * (int64_t)a.Lq * a.D) : nullptr;
  const uint32_t qoff = (uint32_t)(r * a.Lq * a.D + s) * 8u;   // host: 3 Lq D 8 + 1 KB < 2^31
  auto flush_E = [&](int n) {          // rows row_first .. row_first + n - 1 from lanes 0 .. n-1 of each row
    const int first = kRowLanes - n;   // the n parked values sit in lanes 16 - n .. 15, oldest first
    if (valid && s >= first) {
      const int64_t rowb = (int64_t)(row_first - first) * 8;
      if (Ecb) __builtin_nontemporal_store(Ebuf, reinterpret_cast<double*>(Ecb + rowb + eoff));
      if (dEcb) __builtin_nontemporal_store(dEbuf, reinterpret_cast<double*>(dEcb + rowb + eoff));
    }
  };
  uint32_t n_acc = 0, n_acc_wu = 0, n_oob = 0;           // per lane, the same in a row's lanes
  uint32_t n_lf = 0, n_lf2 = 0;                          // per lane: L and L^2 of the iterations this lane drew
  int it_base = a.it0 - kRowLanes, draw_L = 0, draw_npmax = 0;
  double draw_lnu = 0.0;

  // (L, 2 log u) of iteration `it` of the row's chain: lane s drew iteration it_base + s.  What does
  // not need the trajectory is done once per draw, for its 16 iterations: the wave's longest
  // trajectory (pairs of steps, the maximum over the four rows, the same in every row), and the
  // L and L^2 tallies of the drawn iterations this launch runs (exact integers; the rows' lanes are
  // summed once at the end of the kernel).
  int L_nxt = 0, np_max = 0;
  double lnu_nxt = 0.0;
  auto fetch_L = [&](int it) {
    if (it - it_base >= kRowLanes) {
      it_base = it;
      const uint4 rr = draw_block(kDrawSlot, (uint32_t)(it + s), gc, a.k0, a.k1);
      draw_L = uniform_int(rr.x, a.L_low, a.L_high);
      const double u = u53(rr.z, rr.w);
      draw_lnu = u > 0.0 ? fast_log(u) : -__builtin_inf();
      draw_lnu *= 2.0;                                   // compared with 2 dE (exact scaling)
      int m = draw_L >> 1;
      m = max(m, __builtin_amdgcn_ds_bpermute(4 * (lane ^ 16), m));
      draw_npmax = max(m, __builtin_amdgcn_ds_bpermute(4 * (lane ^ 32), m));
      const uint32_t Lr = it + s < a.it1 ? (uint32_t)draw_L : 0u;
      n_lf += Lr;
      n_lf2 += __umul24(Lr, Lr);                         // host: L_high < 2^12
    }
    np_max = __builtin_amdgcn_readlane(draw_npmax, it - it_base);
    const int bsrc = (int)(bprow + 4u * (uint32_t)(it - it_base));
    L_nxt = __builtin_amdgcn_ds_bpermute(bsrc, draw_L);
    lnu_nxt = __hiloint2double(__builtin_amdgcn_ds_bpermute(bsrc, __double2hiint(draw_lnu)),
                               __builtin_amdgcn_ds_bpermute(bsrc, __double2loint(draw_lnu)));
  };

  // One iteration from the state in set `a` (role 0: q, role 1: qt) into set `b`, the other one.  `a`
  // is not written: it is the restore point of a rejecting row.  ma / mb are the sets' parts of q.q,
  // Ea the energy of the iteration before and Eb this one's.
  auto iteration = [&](auto post_c, auto role_c, int it) __attribute__((always_inline)) {
    constexpr bool post = decltype(post_c)::value;
    constexpr bool role = decltype(role_c)::value;
    double (&qa)[C] = role ? qt : q;
    double (&qb)[C] = role ? q : qt;
    double& ma = role ? mtl : ml;
    double& mb = role ? ml : mtl;
    double& Ea = role ? Et : Eprev;
    double& Eb = role ? Eprev : Et;
    const bool write_row = post && ((it == a.niter) || (phase == a.thin - 1));
    fetch_L(it);
    const int L = L_nxt;                                  // >= 1 (host)
    const double lnu = lnu_nxt;
    // three-term leapfrog as in hmc_wave.hip; the parity selects are per lane (per row)
    double (&x)[C] = p;
    const uint32_t oddm = (uint32_t)__builtin_amdgcn_sbfe(L, 0, 1);   // all ones where L is odd
    const uint32_t dtlo = __double2loint(a.dt), dthi = __double2hiint(a.dt);
    const double sh = __hiloint2double(__double2hiint(a.h) ^ ((uint32_t)L << 31), __double2loint(a.h));   // -/+ dt/2
    const double sq = __hiloint2double(dthi & oddm, dtlo & oddm);       // dt (odd L) or 0
    const double sx = a.dt - sq;                                        // 0 (odd L) or dt, exact
#pragma unroll
    for (int e = 0; e < C; ++e) {
      double t;
      asm("v_fma_f64 %0, %1, %2, %3" : "=v"(t) : "v"(sh), "v"(qa[e]), "v"(p[e]));
      x[e] = __builtin_fma(-sx, t, qa[e]);               // u[0] (odd L) or u[-1] = u[0] - dt t
      qb[e] = __builtin_fma(sq, t, qa[e]);               // u[1] = u[0] + dt t (odd L) or u[0]
    }
    const int np = L >> 1;                                // paired steps of this row
    // Pairs of steps up to the wave's longest trajectory.  v_cmpx takes the rows that are done out of
    // EXEC (it only ever shrinks inside the loop: a finished row stays finished), one VALU per pair.
    if (np_max > 0) {
      int i;
      asm volatile("s_mov_b32 %[i], 0\n"
                   "1:\n\t"
                   "v_cmpx_lt_i32_e32 vcc, %[i], %[np]\n\t"
                   "v_fma_f64 %[x0], %[c], %[q0], -%[x0]\n\t"
                   "v_fma_f64 %[x1], %[c], %[q1], -%[x1]\n\t"
                   "v_fma_f64 %[x2], %[c], %[q2], -%[x2]\n\t"
                   "v_fma_f64 %[x3], %[c], %[q3], -%[x3]\n\t"
                   "v_fma_f64 %[x4], %[c], %[q4], -%[x4]\n\t"
                   "v_fma_f64 %[x5], %[c], %[q5], -%[x5]\n\t"
                   "v_fma_f64 %[x6], %[c], %[q6], -%[x6]\n\t"
                   "v_fma_f64 %[q0], %[c], %[x0], -%[q0]\n\t"
                   "v_fma_f64 %[q1], %[c], %[x1], -%[q1]\n\t"
                   "v_fma_f64 %[q2], %[c], %[x2], -%[q2]\n\t"
                   "v_fma_f64 %[q3], %[c], %[x3], -%[q3]\n\t"
                   "v_fma_f64 %[q4], %[c], %[x4], -%[q4]\n\t"
                   "v_fma_f64 %[q5], %[c], %[x5], -%[q5]\n\t"
                   "v_fma_f64 %[q6], %[c], %[x6], -%[q6]\n\t"
                   "s_add_i32 %[i], %[i], 1\n\t"
                   "s_cmp_lt_i32 %[i], %[n]\n\t"
                   "s_cbranch_scc1 1b\n\t"
                   "s_mov_b64 exec, -1"
                   : [x0] "+v"(x[0]), [x1] "+v"(x[1]), [x2] "+v"(x[2]), [x3] "+v"(x[3]), [x4] "+v"(x[4]),
                     [x5] "+v"(x[5]), [x6] "+v"(x[6]), [q0] "+v"(qb[0]), [q1] "+v"(qb[1]), [q2] "+v"(qb[2]),
                     [q3] "+v"(qb[3]), [q4] "+v"(qb[4]), [q5] "+v"(qb[5]), [q6] "+v"(qb[6]), [i] "=&s"(i)
                   : [np] "v"(np), [c] "s"(a.lf_c), [n] "s"(np_max)
                   : "vcc", "scc");
    }
    double w[C];
#pragma unroll
    for (int e = 0; e < C; ++e) w[e] = __builtin_fma(a.lf_ch, qb[e], -x[e]);
    mb = rows_sumsq<C>(qb, 0.0);
    const double k1 = __builtin_fma(rows_sumsq<C>(w, 0.0), a.lf_idt2, mb);
    // one reduction for both: lane 7 of the row holds 2 (E1 - E0), lane 15 holds 2 E0 - logc
    const double s2 = row_sum2_l7_l15(k1 - e0l, e0l);
    Eb = __builtin_fma(s2, 0.5, hlogc);                   // the energy: lane 15
    if (write_row) {
      if (nbuf == 0) row_first = row;
      park_rows(Ebuf, dEbuf, Eb, Eb - Ea, lane15);
      // the count moves outside the flush's per-lane branch (a reset inside it would make the
      // count a per-lane value for the compiler)
      const bool full = nbuf + 1 == kRowLanes;
      if (full) flush_E(kRowLanes);
      nbuf = full ? 0 : nbuf + 1;
    }
    if (it + 1 < a.it1) ring_momentum(it + 1);           // p (x) is dead: the next momentum goes into it
    // the test in lane 7 of each row (where the reduction leaves 2 dE; lnu is the same in the row's
    // lanes); the four bits widened to row masks on the SALU
    const uint64_t b7 = (__builtin_amdgcn_ballot_w64(s2 < 0.0) | __builtin_amdgcn_ballot_w64(lnu < -s2)) & kRowLane7;
    const uint64_t accm = (b7 << 9) - (b7 >> 7);
    const uint64_t rej = ~accm;
    if (rej != 0) {                                       // uniform; the rejecting rows take the start state under EXEC
      uint64_t ex;
      asm volatile("s_mov_b64 %[ex], exec\n\t"
                   "s_mov_b64 exec, %[rej]\n\t"
                   "v_mov_b64 %[q0], %[i0]\n\t"
                   "v_mov_b64 %[q1], %[i1]\n\t"
                   "v_mov_b64 %[q2], %[i2]\n\t"
                   "v_mov_b64 %[q3], %[i3]\n\t"
                   "v_mov_b64 %[q4], %[i4]\n\t"
                   "v_mov_b64 %[q5], %[i5]\n\t"
                   "v_mov_b64 %[q6], %[i6]\n\t"
                   "v_mov_b64 %[m1], %[m0]\n\t"
                   "s_mov_b64 exec, %[ex]"
                   : [q0] "+v"(qb[0]), [q1] "+v"(qb[1]), [q2] "+v"(qb[2]), [q3] "+v"(qb[3]), [q4] "+v"(qb[4]),
                     [q5] "+v"(qb[5]), [q6] "+v"(qb[6]), [m1] "+v"(mb), [ex] "=&s"(ex)
                   : [rej] "s"(rej), [i0] "v"(qa[0]), [i1] "v"(qa[1]), [i2] "v"(qa[2]), [i3] "v"(qa[3]),
                     [i4] "v"(qa[4]), [i5] "v"(qa[5]), [i6] "v"(qa[6]), [m0] "v"(ma));
    }
    if (write_row && qcb && row >= a.q_row0) {
      char* const rowb = qcb + (int64_t)qslot * a.D * 8;
#pragma unroll
      for (int j = 0; j < C; ++j)
        if (j < C - 1 ? valid : st6)
          __builtin_nontemporal_store(qb[j], reinterpret_cast<double*>(rowb + qoff) + kRowLanes * j);
    }
    if (post) add_mask(n_acc, accm); else add_mask(n_acc_wu, accm);
    // a rejection before i_oob = wu - Lc thin <= wu: only the warm-up instance can meet one
    if constexpr (!post) add_mask(n_oob, it < a.i_oob ? rej : 0ull);
    e0l = rows_sumsq<C>(p, mb);                           // the state kept is in set b
    if (post && ++phase == a.thin) {
      phase = 0;
      ++row;
      if (++qslot == a.Lq) qslot = 0;
    }
  };
  const int it_mid = min(max(a.wu, a.it0), a.it1);
  // Two iterations per trip, one in each role.  A loop that ends after an odd number of iterations
  // leaves the state in the second set: it is copied back once, so both loops start and the kernel
  // ends in role 0.
  auto iterations = [&](auto post_c, int from, int to) __attribute__((always_inline)) {
    int it = from;
    for (; it + 1 < to; it += 2) {
      iteration(post_c, std::false_type{}, it);
      iteration(post_c, std::true_type{}, it + 1);
    }
    if (it < to) {
      iteration(post_c, std::false_type{}, it);
#pragma unroll
      for (int e = 0; e < C; ++e) q[e] = qt[e];
      ml = mtl;
      Eprev = Et;
    }
  };
  iterations(std::false_type{}, a.it0, it_mid);
  iterations(std::true_type{}, it_mid, a.it1);

  if (nbuf > 0) flush_E(nbuf);
#pragma unroll
  for (int j = 0; j < C; ++j)
    if (j < C - 1 ? valid : st6) reinterpret_cast<double*>(qstb + qstoff)[kRowLanes * j] = q[j];
  n_lf = row_sum_u32_l15(n_lf);
  n_lf2 = row_sum_u32_l15(n_lf2);
  if (valid && s == kRowLanes - 1) {                      // lane 15: where the row sums leave E and the tallies
    reinterpret_cast<double*>(reinterpret_cast<char*>(a.Eprev + c0) + 8u * r)[0] = Eprev;
    if (a.cnt) {
      unsigned long long* cs = a.cnt + (c & (HMC_COUNTER_SLOTS - 1)) * HMC_NCOUNTERS;
      if (n_acc) atomicAdd(cs + HMC_CNT_ACCEPT, (unsigned long long)n_acc);
      if (n_acc_wu) atomicAdd(cs + HMC_CNT_ACCEPT_WU, (unsigned long long)n_acc_wu);
      if (n_lf) atomicAdd(cs + HMC_CNT_LEAPFROG, (unsigned long long)n_lf);
      if (n_lf2) atomicAdd(cs + HMC_CNT_LEAPFROG_SQ, (unsigned long long)n_lf2);
      if (n_oob) atomicAdd(cs + HMC_CNT_OOB_REJECT, (unsigned long long)n_oob);
    }
  }
}

}  // namespace

hipError_t launch_rows_iters(const RandArgs& a, hipStream_t s) {
  // more than 64 KB of LDS: the limit is raised once per device
  static bool raised[64] = {};
  int dev = 0;
  if (hipError_t e = hipGetDevice(&dev)) return e;
  if (dev < 0 || dev >= 64 || !raised[dev]) {
    // the kernel addresses its dynamic LDS from byte 0: it must have no static LDS in front of it
    hipFuncAttributes fa;
    if (hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_rows_iters<7>))) return e;
    if (fa.sharedSizeBytes != 0) return hipErrorInvalidConfiguration;
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rows_iters<7>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRowsLds))
      return e;
    if (dev >= 0 && dev < 64) raised[dev] = true;
  }
  constexpr int chains_per_block = (kRowsBlock / kWave) * kRowChains;
  const dim3 grid((unsigned)((a.n + chains_per_block - 1) / chains_per_block));
  k_rows_iters<7><<<grid, kRowsBlock, kRowsLds, s>>>(a);
  return hipGetLastError();
}

}  // namespace hmc
