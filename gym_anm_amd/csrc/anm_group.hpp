// anm_group.hpp -- lane-group Newton-Raphson for a compile-time TREE topology (gfx950 only).
//
// Why: a diverging power flow runs to the reference's iteration cap (100, solve_load_flow.py:176) while
// every converging solve of the batch is done after <= 9 iterations.  In the thread-per-environment
// kernels such a solve keeps ONE lane of its wavefront busy for ~90 more trips of ~500-665 fp64
// instructions each: the launch time of the headline configuration (65 536 environments = one wave
// per SIMD) is exactly that serial chain.  Here a solve that is still running after `handoff_after`
// iterations leaves its lane and continues spread over a group of G lanes of the same wavefront,
//     lane l of the group  <->  bus l + 1  (and the branch joining it to its parent bus),
// so that one trip costs the wavefront ~1/3 of the instructions: every lane forms the three W products
// of its own tree edge, the tree is eliminated by height (all leaves at once, then their parents, ...)
// and back-substituted by depth.  Hand-overs between lanes are register-to-register where the tree allows
// it (DPP row shifts, else `ds_bpermute_b32`: nothing is stored anywhere inside the loop) or go through LDS
// slots (the radial kernel's larger trees, see LDSX below).  Everything structural (parent, children, height, depth of each bus, position of its admittances
// in the constant buffer) is a constexpr table of the Topo descriptor (codegen.py: tree_tables), so the
// level loops are unrolled and a level only pulls as many child slots as a bus of that height can have.
//
// Same reference semantics and the same formulation as the thread-per-environment kernels (W_ik =
// V_i conj(Y_ik V_k), magnitude columns scaled by |V|, rotated loop, (cos, sin) state: see
// anm_device.hpp); results differ from them by summation order only (~1e-16).  Reference:
//   _newton_raphson_sparse / _f / _dfdx   gym_anm/simulator/solve_load_flow.py:84-226
#pragma once

#include "anm_device.hpp"

#if defined(__HIPCC__)
namespace anm {
namespace group {

// iteration up to which a wavefront with more handed-over solves than rows keeps them on groups (continue_collective), and
// where the first straggler launch leaves the solves still running to the second (anm_capi.hip)
#ifndef ANM_MID_CAP_DEFAULT
#define ANM_MID_CAP_DEFAULT 12
#endif

constexpr int LDSX_FETCH = 3;   // child slots a parent lane fetches from LDS before folding them (LDS hand-overs)

// llvm CmpInst predicate codes taken by __builtin_amdgcn_{fcmp,uicmp,sicmp}: they return the compare as a
// 64-bit lane mask in scalar registers (no bool -> ballot round trip)
enum : int { FCMP_UNO = 8, FCMP_UGT = 10, ICMP_EQ = 32, ICMP_NE = 33, ICMP_SLT = 40 };

// ---------------------------------------------------------------------------------------------
// Hand-overs between the lanes of a group.  Two register-to-register implementations behind one interface,
// chosen per topology by codegen.dpp_plan (a third one, through LDS slots, lives in newton_groups<.., LDSX>):
//   * DPP row shifts (v_mov_b32_dpp row_shl/row_shr + bank mask): no latency to wait for, when the tree has
//     a lane layout in which every hand-over class is at most two whole-row shifts;
//   * ds_bpermute_b32 (the LDS crossbar, no LDS memory): any tree, ~100 cycles of latency per hand-over.
// Both rely on the PADDING lanes of a group (there is always at least one) holding neutral values in every
// group of the wavefront -- V = 1 + 0j, W = 0, Schur complement 0, step 0 -- so that "the parent of a bus
// attached to the slack" and "a child this bus does not have" are ordinary sources: no selects.
// Every lane of the wavefront must be executing at a hand-over.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double bperm(double x, int src4) {
  const int lo = __builtin_amdgcn_ds_bpermute(src4, __double2loint(x));
  const int hi = __builtin_amdgcn_ds_bpermute(src4, __double2hiint(x));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float bperm(float x, int src4) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(x)));
}
// One DPP move of x.  FULL: whole-row move with bound_ctrl (lanes shifted in from outside the row read 0).
// FIRST && !FULL: a bank-masked move with nothing to merge into -- the lanes it does not write are left
// UNDEFINED (no register to initialise); the caller only consumes it on the lanes that have a source.
template <int CTRL, int BANK, int FULL, bool FIRST>
__device__ __forceinline__ int dpp_move32(int old, int x) {
  if constexpr (FIRST) {
    (void)old;
    return __builtin_amdgcn_mov_dpp(x, CTRL, 0xF, FULL ? 0xF : BANK, FULL != 0);
  } else {
    return __builtin_amdgcn_update_dpp(old, x, CTRL, 0xF, BANK, false);
  }
}
template <int CTRL, int BANK, int FULL, bool FIRST>
__device__ __forceinline__ double dpp_move(double old, double x) {
  const int lo = dpp_move32<CTRL, BANK, FULL, FIRST>(__double2loint(old), __double2loint(x));
  const int hi = dpp_move32<CTRL, BANK, FULL, FIRST>(__double2hiint(old), __double2hiint(x));
  return __hiloint2double(hi, lo);
}
template <int CTRL, int BANK, int FULL, bool FIRST>
__device__ __forceinline__ float dpp_move(float old, float x) {
  return __int_as_float(dpp_move32<CTRL, BANK, FULL, FIRST>(__float_as_int(old), __float_as_int(x)));
}

template <class T>
struct Lanes {
  int psrc4;               // bpermute address of the parent's lane (roots, padding lanes: a padding lane)
  int csrc4[T::T_MAXCH];   // ... of the c-th child's lane (no such child: a padding lane)

  // x as held by the lane of this lane's parent bus (a bus attached to the slack, a padding lane: what a
  // padding lane holds, `neutral`)
  template <class R>
  __device__ __forceinline__ R from_parent(R x, R neutral) const {
    if constexpr (T::T_DPP != 0) {
      R v = neutral;
      if constexpr (T::T_PAR_N > 0) {
        static_assert(T::T_PAR_FULL[0] != 0, "codegen.dpp_plan: the first parent move covers the whole row");
        v = dpp_move<T::T_PAR_CTRL[0], T::T_PAR_BANK[0], 1, true>(v, x);
      }
      if constexpr (T::T_PAR_N > 1) v = dpp_move<T::T_PAR_CTRL[1], T::T_PAR_BANK[1], 0, false>(v, x);
      return v;
    } else {
      return bperm(x, psrc4);
    }
  }
  // does from_child<CH> deliver the neutral 0 on the lanes without such a child?  (else: undefined there)
  template <int CH>
  static constexpr bool child_neutral() {
    return T::T_DPP == 0 || T::T_CH_N[CH] == 0 || T::T_CH_FULL[2 * CH] != 0;
  }
  // x as held by the lane of this lane's CH-th child
  template <int CH, class R>
  __device__ __forceinline__ R from_child(R x) const {
    if constexpr (T::T_DPP != 0) {
      R v = R(0);
      if constexpr (T::T_CH_N[CH] > 0)
        v = dpp_move<T::T_CH_CTRL[2 * CH], T::T_CH_BANK[2 * CH], T::T_CH_FULL[2 * CH], true>(v, x);
      if constexpr (T::T_CH_N[CH] > 1)
        v = dpp_move<T::T_CH_CTRL[2 * CH + 1], T::T_CH_BANK[2 * CH + 1], 0, false>(v, x);
      return v;
    } else {
      return bperm(x, csrc4[CH]);
    }
  }
};

template <class T>
constexpr int first_padding_lane() {
  for (int l = 0; l < T::GRP; ++l)
    if (T::T_LANE_BUS[l] == 0) return l;
  return -1;
}

// Which buses fold their c-th child at elimination level h (the child has height h - 1) -- of the buses of height h:
// 2 = every one, 1 = some, 0 = none; and: does a bus of a GREATER height fold a c-th child there (an "early" fold: the child
// is folded at the level right after its own, whatever the height of its parent).  Bus 0 (the slack) folds nothing.
template <class T>
constexpr int fold_at_own_level(int h, int c) {
  int n = 0, k = 0;
  for (int b = 1; b < T::NB; ++b)
    if (T::T_HEIGHT[b] == h) {
      ++n;
      const int ch = T::T_CH[b * T::T_MAXCH + c];
      if (ch > 0 && T::T_HEIGHT[ch] == h - 1) ++k;
    }
  return k == 0 ? 0 : (k == n ? 2 : 1);
}
template <class T>
constexpr bool fold_early(int h, int c) {
  for (int b = 1; b < T::NB; ++b)
    if (T::T_HEIGHT[b] > h) {
      const int ch = T::T_CH[b * T::T_MAXCH + c];
      if (ch > 0 && T::T_HEIGHT[ch] == h - 1) return true;
    }
  return false;
}
// do the moves of all child classes write the same lanes of a row?  (one loop-carried register then receives them all in turn)
template <class T>
constexpr bool child_moves_write_the_same_lanes() {
  if (T::T_DPP == 0) return false;
  unsigned first = 0u;
  for (int c = 0; c < T::T_MAXCH; ++c) {
    const int ctrl = T::T_CH_CTRL[2 * c], bank = T::T_CH_BANK[2 * c], k = ctrl & 0xF;
    const bool shl = (ctrl & 0x1F0) == 0x100;
    unsigned m = 0u;
    for (int l = 0; l < 16; ++l) {
      const int sl = shl ? l + k : l - k;
      if (((bank >> (l / 4)) & 1) != 0 && sl >= 0 && sl <= 15) m |= 1u << l;
    }
    if (c == 0) first = m;
    else if (m != first) return false;
  }
  return true;
}
// of the buses of height h: 2 = every one hangs off the slack (depth 0), 1 = some, 0 = none
template <class T>
constexpr int roots_at_height(int h) {
  int n = 0, k = 0;
  for (int b = 1; b < T::NB; ++b)
    if (T::T_HEIGHT[b] == h) {
      ++n;
      if (T::T_DEPTH[b] == 0) ++k;
    }
  return k == 0 ? 0 : (k == n ? 2 : 1);
}
// Child sums without a predicate: the move of child class c (ONE bank-masked row shift, written into a register that is
// zero on the lanes the move never writes and keeps them so) delivers to every bus lane it writes either the value of that
// bus's c-th child or that of a padding lane -- whose W product is zero: its admittances are.  Checked lane by lane over a
// 16-lane row; a shift that would cross into the row's other group must read a padding lane there too.
template <class T>
constexpr bool child_moves_land_on_parents_or_zero() {
  if (T::T_DPP == 0 || T::GRP > 16) return false;
  for (int c = 0; c < T::T_MAXCH; ++c) {
    if (T::T_CH_N[c] != 1 || T::T_CH_FULL[2 * c] != 0) return false;
    const int ctrl = T::T_CH_CTRL[2 * c], bank = T::T_CH_BANK[2 * c];
    const int k = ctrl & 0xF, shl = (ctrl & 0x1F0) == 0x100, shr = (ctrl & 0x1F0) == 0x110;
    if (!shl && !shr) return false;
    for (int l = 0; l < 16; ++l) {
      if (((bank >> (l / 4)) & 1) == 0) continue;
      const int sl = shl ? l + k : l - k;
      if (sl < 0 || sl > 15) continue;                       // no source: not written
      const int R = T::T_LANE_BUS[l % T::GRP], S = T::T_LANE_BUS[sl % T::GRP];
      if (R == 0) continue;                                  // a padding lane receives: nobody reads its sums
      if (S == 0) {
        // a padding lane's product arrives: 0 x (the voltage of whatever lane its own "parent" moves read) -- a zero unless
        // that voltage is Inf / NaN, so that lane must belong to the receiver's environment (whose solve is lost then
        // anyway), never to the neighbouring group of the row
        int src = -1;
        for (int m = 0; m < T::T_PAR_N; ++m) {
          const int pc = T::T_PAR_CTRL[m], pk = pc & 0xF;
          const bool pshl = (pc & 0x1F0) == 0x100, pshr = (pc & 0x1F0) == 0x110;
          if (!pshl && !pshr) return false;
          if (T::T_PAR_FULL[m] == 0 && ((T::T_PAR_BANK[m] >> (sl / 4)) & 1) == 0) continue;
          const int q = pshl ? sl + pk : sl - pk;
          if (q < 0 || q > 15) { if (T::T_PAR_FULL[m] != 0) src = -1; continue; }
          src = q;
        }
        if (src >= 0 && src / T::GRP != l / T::GRP) return false;
        continue;
      }
      if (l / T::GRP != sl / T::GRP) return false;           // another environment's bus
      if (T::T_CH[R * T::T_MAXCH + c] != S) return false;
    }
  }
  // ... and every bus's c-th child IS delivered by that move
  for (int b = 1; b < T::NB; ++b)
    for (int c = 0; c < T::T_MAXCH; ++c) {
      const int ch = T::T_CH[b * T::T_MAXCH + c];
      if (ch <= 0) continue;
      const int ctrl = T::T_CH_CTRL[2 * c], bank = T::T_CH_BANK[2 * c], k = ctrl & 0xF;
      const int l = T::T_POS[b], sl = ((ctrl & 0x1F0) == 0x100) ? l + k : l - k;
      if (((bank >> (l / 4)) & 1) == 0 || sl < 0 || sl >= T::GRP || T::T_LANE_BUS[sl] != ch) return false;
    }
  return true;
}

// ---------------------------------------------------------------------------------------------
// Hand-overs inside a 16-lane row that holds ONE solve, one lane per bus (codegen.row_plan; newton_rows below): gfx950's
// two 64-bit DPP forms,
//     v_fmac_f64_dpp d, -s, m  row_newbcast:N row_mask:0xf bank_mask:B     d += -(s of lane N of my row) * m
//     v_mov_b64_dpp  d,  s     row_newbcast:N row_mask:0xf bank_mask:B     d  =   s of lane N of my row
// on the lanes of the banks (4 consecutive lanes) B names; every other lane keeps its d.  A hand-over and the operation
// that folds the moved value in are one instruction: `D -= x_child` is fmac(D, -x, 1.0) -- the product by 1 is exact, one
// rounding, the bits of the subtraction -- and `a = fma(-J, p_parent, a)` is fmac(a, -p, J), the same product.
// Two rules these statements keep, because nothing else does:
//   * the compiler inserts no wait states in front of inline-asm DPP, and a DPP read of a register needs two of them behind
//     the VALU write of it.  A statement therefore opens with a LEAD of at least two instructions that are no DPP reads, and
//     no DPP read of a statement follows the write of its source, inside the statement, by fewer than two instructions:
//     whatever the compiler wrote last in front of the statement is then two instructions away as well.  The lead is the
//     trip's own arithmetic that stands in front of the hand-over anyway (row_*_lead: the same single v_mul / v_add /
//     v_fmac the compiler makes of the source expression, the same operands in the same order), so the wait states cost no
//     issue slot.  Where a hand-over point needs more than one statement, those behind the first (row_mov, row_wsum,
//     row_fold, row_fma) have no arithmetic left to lead with and open with `s_nop 1`;
//   * a source lane switched off by EXEC is not read: every lane of the wavefront executes them (asm volatile: not sunk
//     into a divergent region).
// One statement serves up to four hand-overs of one point -- they read the same registers -- so a point has one lead, not
// one per hand-over.  A hand-over is a (source lane N, second source lane M, bank mask B) triple: M is named by the fold
// on two lanes per bus alone (ANM_ROW2_FOLD6), every other body reads lane N only, so a statement's template arguments are
// the (N, B) pairs followed by the M's, which default to none.  (N1 / N2 / N3 < 0: no such hand-over.)
// A statement is LEAD(F) followed by BODY(F, n, m, b) per hand-over, F the "f64" / "f32" of the element type (ANM_ROW_ASM_T
// chooses it; the voltage and W statements are f64 only).
// ---------------------------------------------------------------------------------------------
#define ANM_ROW_CTL(n, b) " row_newbcast:%[" n "] row_mask:0xf bank_mask:%[" b "]\n"
#define ANM_ROW_INTS                                                                                                   \
  int N0, int B0, int N1 = -1, int B1 = 0, int N2 = -1, int B2 = 0, int N3 = -1, int B3 = 0, int M0 = -1, int M1 = -1,   \
      int M2 = -1, int M3 = -1
#define ANM_ROW_IMM                                                                                                    \
  [n0] "n"(N0), [k0] "n"(M0 < 0 ? 0 : M0), [b0] "n"(B0), [n1] "n"(N1 < 0 ? 0 : N1), [k1] "n"(M1 < 0 ? 0 : M1),            \
  [b1] "n"(B1), [n2] "n"(N2 < 0 ? 0 : N2), [k2] "n"(M2 < 0 ? 0 : M2), [b2] "n"(B2), [n3] "n"(N3 < 0 ? 0 : N3),           \
  [k3] "n"(M3 < 0 ? 0 : M3), [b3] "n"(B3)
#define ANM_ROW_UNPAR(...) __VA_ARGS__
#define ANM_ROW_ASM(F, LEAD, BODY, OUTS, INS)                                                                           \
  do {                                                                                                                 \
    if constexpr (N1 < 0) asm volatile(LEAD(F) BODY(F, "n0", "k0", "b0") : ANM_ROW_UNPAR OUTS : ANM_ROW_UNPAR INS, ANM_ROW_IMM); \
    else if constexpr (N2 < 0)                                                                                         \
      asm volatile(LEAD(F) BODY(F, "n0", "k0", "b0") BODY(F, "n1", "k1", "b1") : ANM_ROW_UNPAR OUTS                      \
                   : ANM_ROW_UNPAR INS, ANM_ROW_IMM);                                                                  \
    else if constexpr (N3 < 0)                                                                                         \
      asm volatile(LEAD(F) BODY(F, "n0", "k0", "b0") BODY(F, "n1", "k1", "b1") BODY(F, "n2", "k2", "b2")                 \
                   : ANM_ROW_UNPAR OUTS : ANM_ROW_UNPAR INS, ANM_ROW_IMM);                                             \
    else                                                                                                               \
      asm volatile(LEAD(F) BODY(F, "n0", "k0", "b0") BODY(F, "n1", "k1", "b1") BODY(F, "n2", "k2", "b2")                 \
                   BODY(F, "n3", "k3", "b3") : ANM_ROW_UNPAR OUTS : ANM_ROW_UNPAR INS, ANM_ROW_IMM);                    \
  } while (0)
#define ANM_ROW_ASM_T(R, LEAD, BODY, OUTS, INS)                                                                         \
  do {                                                                                                                 \
    if constexpr (std::is_same_v<R, double>) ANM_ROW_ASM("f64", LEAD, BODY, OUTS, INS);                                 \
    else ANM_ROW_ASM("f32", LEAD, BODY, OUTS, INS);                                                                     \
  } while (0)
#define ANM_ROW_MOV2(F, n, m, b) "v_mov_b64_dpp %[d0], %[s0]" ANM_ROW_CTL(n, b) "v_mov_b64_dpp %[d1], %[s1]" ANM_ROW_CTL(n, b)
#define ANM_ROW_WSUM(F, n, m, b) "v_fmac_f64_dpp %[d0], %[s0], %[one]" ANM_ROW_CTL(n, b) "v_fmac_f64_dpp %[d1], -%[s1], %[one]" ANM_ROW_CTL(n, b)
#define ANM_ROW_FOLD6(F, n, m, b)                                                                                    \
  "v_fmac_" F "_dpp %[a], -%[sa], %[one]" ANM_ROW_CTL(n, b) "v_fmac_" F "_dpp %[b], -%[sb], %[one]" ANM_ROW_CTL(n, b)  \
  "v_fmac_" F "_dpp %[c], -%[sc], %[one]" ANM_ROW_CTL(n, b) "v_fmac_" F "_dpp %[d], -%[sd], %[one]" ANM_ROW_CTL(n, b)  \
  "v_fmac_" F "_dpp %[r0], -%[l0], %[one]" ANM_ROW_CTL(n, b) "v_fmac_" F "_dpp %[r1], -%[l1], %[one]" ANM_ROW_CTL(n, b)
#define ANM_ROW_FMA4(F, n, m, b)                                                                                     \
  "v_fmac_" F "_dpp %[a0], -%[p0], %[ja]" ANM_ROW_CTL(n, b) "v_fmac_" F "_dpp %[a1], %[p0], %[jb]" ANM_ROW_CTL(n, b)   \
  "v_fmac_" F "_dpp %[a0], -%[p1], %[jb]" ANM_ROW_CTL(n, b) "v_fmac_" F "_dpp %[a1], -%[p1], %[ja]" ANM_ROW_CTL(n, b)
// The fold on TWO lanes per bus (codegen.row_pair_plan; newton_rows<.., PAIRS>): lane N holds row 0 of the child's Schur
// complement and reduced right-hand side -- (s0, s1, l) = (Sc.a, Sc.b, Lr0) -- and lane M row 1, (Sc.c, Sc.d, Lr1), in the
// SAME three registers.  Six instructions per hand-over like ANM_ROW_FOLD6, the same six subtractions.
#define ANM_ROW2_FOLD6(F, n, m, b)                                                                                   \
  "v_fmac_" F "_dpp %[a], -%[s0], %[one]" ANM_ROW_CTL(n, b) "v_fmac_" F "_dpp %[c], -%[s0], %[one]" ANM_ROW_CTL(m, b)  \
  "v_fmac_" F "_dpp %[b], -%[s1], %[one]" ANM_ROW_CTL(n, b) "v_fmac_" F "_dpp %[d], -%[s1], %[one]" ANM_ROW_CTL(m, b)  \
  "v_fmac_" F "_dpp %[r0], -%[l], %[one]" ANM_ROW_CTL(n, b) "v_fmac_" F "_dpp %[r1], -%[l], %[one]" ANM_ROW_CTL(m, b)
// The leads (the first rule above; the distances are counted in instructions of the statement, lead included):
//   ANM_ROW_LEAD_NOP   a statement behind the first of its point
//   ANM_ROW_LEAD_MOV   vr = vm cs, vi = vm sn, m2 = vm^2, then the moves: vr is read at distance 2, vi at distance 2
//   ANM_ROW_LEAD_WSUM  the two additions that start the sums, then the children's products (no DPP read of a lead result)
//   ANM_ROW_LEAD_FOLD  l0 += ka r0, l1 += kc r0 (the fmacs that finish Lr = Lk r), then the six folds: l0 / l1 at distance 5
//   ANM_ROW2_LEAD_FOLD s1 += ka jb, l += ka r0 (the fmacs that finish my row of Sc = Lk Jbp and my entry of Lr = Lk r; s1 comes
//                      in holding kb Jbp.d, l holding kb r1), then the folds, those of s0 first: s1 at distance 4, l at distance 5
//   ANM_ROW_LEAD_STEP  p = Di r as mul, fmac (p0), mul, fmac (p1), then the four fused steps, which read p0, p0, p1, p1: each at
//                      distance 2.  (r0 / r1 are read by the lead and accumulated into by the steps.)
#define ANM_ROW_LEAD_NOP(F) "s_nop 1\n"
#define ANM_ROW_LEAD_MOV(F) "v_mul_f64 %[s0], %[vm], %[cs]\nv_mul_f64 %[s1], %[vm], %[sn]\nv_mul_f64 %[m2], %[vm], %[vm]\n"
#define ANM_ROW_LEAD_WSUM(F) "v_add_f64 %[d0], %[x0], %[y0]\nv_add_f64 %[d1], %[x1], %[y1]\n"
#define ANM_ROW_LEAD_FOLD(F) "v_fmac_" F " %[l0], %[ka], %[r0]\nv_fmac_" F " %[l1], %[kc], %[r0]\n"
#define ANM_ROW2_LEAD_FOLD(F) "v_fmac_" F " %[s1], %[ka], %[jb]\nv_fmac_" F " %[l], %[ka], %[r0]\n"
#define ANM_ROW_LEAD_STEP(F)                                                                                     \
  "v_mul_" F " %[p0], %[a1], %[ib]\nv_fmac_" F " %[p0], %[ia], %[a0]\nv_mul_" F " %[p1], %[a1], %[id]\nv_fmac_" F  \
  " %[p1], %[ic], %[a0]\n"

// (d0, d1) = (s0, s1) of lane N: the parent's voltage
template <ANM_ROW_INTS>
__device__ __forceinline__ void row_mov(double& d0, double& d1, double s0, double s1) {
  ANM_ROW_ASM("f64", ANM_ROW_LEAD_NOP, ANM_ROW_MOV2, ([d0] "+v"(d0), [d1] "+v"(d1)), ([s0] "v"(s0), [s1] "v"(s1)));
}
// (vr, vi, m2) = (vm cs, vm sn, vm^2), then row_mov of (vr, vi)
template <ANM_ROW_INTS>
__device__ __forceinline__ void row_mov_lead(double& d0, double& d1, double& vr, double& vi, double& m2, double vm, double cs, double sn) {
  ANM_ROW_ASM("f64", ANM_ROW_LEAD_MOV, ANM_ROW_MOV2, ([d0] "+v"(d0), [d1] "+v"(d1), [s0] "=&v"(vr), [s1] "=&v"(vi), [m2] "=&v"(m2)),
              ([vm] "v"(vm), [cs] "v"(cs), [sn] "v"(sn)));
}
// d0 += s0 of lane N, d1 -= s1 of lane N: a child's W product into its parent's sum (`one` holds 1.0)
template <ANM_ROW_INTS>
__device__ __forceinline__ void row_wsum(double& d0, double& d1, double s0, double s1, double one) {
  ANM_ROW_ASM("f64", ANM_ROW_LEAD_NOP, ANM_ROW_WSUM, ([d0] "+v"(d0), [d1] "+v"(d1)), ([s0] "v"(s0), [s1] "v"(s1), [one] "v"(one)));
}
// (d0, d1) = (x0 + y0, x1 + y1), then row_wsum
template <ANM_ROW_INTS>
__device__ __forceinline__ void row_wsum_lead(double& d0, double& d1, double x0, double y0, double x1, double y1, double s0, double s1,
                                              double one) {
  ANM_ROW_ASM("f64", ANM_ROW_LEAD_WSUM, ANM_ROW_WSUM, ([d0] "=&v"(d0), [d1] "=&v"(d1)),
              ([x0] "v"(x0), [y0] "v"(y0), [x1] "v"(x1), [y1] "v"(y1), [s0] "v"(s0), [s1] "v"(s1), [one] "v"(one)));
}
// D -= Sc of lane N, (r0, r1) -= (l0, l1) of lane N: a child's Schur complement and reduced right-hand side into its parent
template <ANM_ROW_INTS, class R>
__device__ __forceinline__ void row_fold(Blk<R>& D, R& r0, R& r1, const Blk<R>& Sc, R l0, R l1, R one) {
  ANM_ROW_ASM_T(R, ANM_ROW_LEAD_NOP, ANM_ROW_FOLD6, ([a] "+v"(D.a), [b] "+v"(D.b), [c] "+v"(D.c), [d] "+v"(D.d), [r0] "+v"(r0), [r1] "+v"(r1)),
                ([sa] "v"(Sc.a), [sb] "v"(Sc.b), [sc] "v"(Sc.c), [sd] "v"(Sc.d), [l0] "v"(l0), [l1] "v"(l1), [one] "v"(one)));
}
// (l0, l1) += (ka, kc) r0 -- they come in holding (kb, kd) r1 -- then row_fold
template <ANM_ROW_INTS, class R>
__device__ __forceinline__ void row_fold_lead(Blk<R>& D, R& r0, R& r1, const Blk<R>& Sc, R& l0, R& l1, R ka, R kc, R one) {
  ANM_ROW_ASM_T(R, ANM_ROW_LEAD_FOLD, ANM_ROW_FOLD6,
                ([a] "+v"(D.a), [b] "+v"(D.b), [c] "+v"(D.c), [d] "+v"(D.d), [r0] "+v"(r0), [r1] "+v"(r1), [l0] "+v"(l0), [l1] "+v"(l1)),
                ([sa] "v"(Sc.a), [sb] "v"(Sc.b), [sc] "v"(Sc.c), [sd] "v"(Sc.d), [ka] "v"(ka), [kc] "v"(kc), [one] "v"(one)));
}
// row_fold on two lanes per bus: D's row 0 and r0 -= (s0, s1, l) of lane N, row 1 and r1 -= those of lane M
template <ANM_ROW_INTS, class R>
__device__ __forceinline__ void row_pair_fold(Blk<R>& D, R& r0, R& r1, R s0, R s1, R l, R one) {
  ANM_ROW_ASM_T(R, ANM_ROW_LEAD_NOP, ANM_ROW2_FOLD6, ([a] "+v"(D.a), [b] "+v"(D.b), [c] "+v"(D.c), [d] "+v"(D.d), [r0] "+v"(r0), [r1] "+v"(r1)),
                ([s0] "v"(s0), [s1] "v"(s1), [l] "v"(l), [one] "v"(one)));
}
// s1 += ka jb, l += ka r0, then row_pair_fold
template <ANM_ROW_INTS, class R>
__device__ __forceinline__ void row_pair_fold_lead(Blk<R>& D, R& r0, R& r1, R s0, R& s1, R& l, R ka, R jb, R one) {
  ANM_ROW_ASM_T(R, ANM_ROW2_LEAD_FOLD, ANM_ROW2_FOLD6,
                ([a] "+v"(D.a), [b] "+v"(D.b), [c] "+v"(D.c), [d] "+v"(D.d), [r0] "+v"(r0), [r1] "+v"(r1), [s1] "+v"(s1), [l] "+v"(l)),
                ([s0] "v"(s0), [ka] "v"(ka), [jb] "v"(jb), [one] "v"(one)));
}
// a0 = fma(-J.b, p1 of lane N, fma(-J.a, p0 of lane N, a0)), a1 likewise with (J.c, J.d): the parent's Newton step into
// the right-hand side of the back substitution.  The block is a coupling block of the polar Jacobian, {ja, jb, -jb, ja}
// (Jbp of newton_rows): the statement takes ja and jb alone and forms the product by J.c = -jb as +(p0 * jb) -- the sign
// of a product is the exclusive or of its factors' signs, the magnitude is the same, so the bits are those of -p0 * -jb.
template <ANM_ROW_INTS, class R>
__device__ __forceinline__ void row_fma(R& a0, R& a1, R p0, R p1, R ja, R jb) {
  ANM_ROW_ASM_T(R, ANM_ROW_LEAD_NOP, ANM_ROW_FMA4, ([a0] "+v"(a0), [a1] "+v"(a1)), ([p0] "v"(p0), [p1] "v"(p1), [ja] "v"(ja), [jb] "v"(jb)));
}
// (p0, p1) = Di (r0, r1) -- a lane's own Newton step -- then row_fma with it: the step of a parent into its children
template <ANM_ROW_INTS, class R>
__device__ __forceinline__ void row_step_lead(R& r0, R& r1, R& p0, R& p1, const Blk<R>& Di, R ja, R jb) {
  ANM_ROW_ASM_T(R, ANM_ROW_LEAD_STEP, ANM_ROW_FMA4, ([a0] "+v"(r0), [a1] "+v"(r1), [p0] "=&v"(p0), [p1] "=&v"(p1)),
                ([ia] "v"(Di.a), [ib] "v"(Di.b), [ic] "v"(Di.c), [id] "v"(Di.d), [ja] "v"(ja), [jb] "v"(jb)));
}
// Two integer statements of the stop test that the compiler makes longer than the instruction set needs:
//   row_count   it + 1 on the lanes of the wavefront mask m, it elsewhere: ONE add with carry-in (select and add: two)
//   row_pick    (lo(m) & glo) | (hi(m) & ghi): v_and_b32 + v_and_or_b32 (and, and, or: three)
// Both depend on wave64: m is a 64-bit lane mask in an SGPR pair (row_count's carry-in and carry-out are such pairs; each
// VOP3 names one SGPR source, the limit of gfx9).  row_pick makes no assumption about where the lanes of glo / ghi lie; its
// callers pass a row's bus lanes, which lie in one half of the wavefront, so one of the two terms is zero.
__device__ __forceinline__ int row_count(int it, unsigned long long m) {
  int d;
  unsigned long long carry_out;
  asm("v_addc_co_u32_e64 %[d], %[co], 0, %[a], %[m]" : [d] "=v"(d), [co] "=s"(carry_out) : [a] "v"(it), [m] "s"(m));
  return d;
}
__device__ __forceinline__ unsigned row_pick(unsigned long long m, unsigned glo, unsigned ghi) {
  unsigned t, d;
  asm("v_and_b32 %[t], %[hi], %[ghi]\nv_and_or_b32 %[d], %[lo], %[glo], %[t]"
      : [t] "=&v"(t), [d] "=v"(d)
      : [lo] "s"(unsigned(m)), [hi] "s"(unsigned(m >> 32)), [glo] "v"(glo), [ghi] "v"(ghi));
  return d;
}
// the tables of codegen.row_plan: PAR (parent -> children), CH (child -> parent, by level), WS (child -> parent, by parent);
// CH_PAIR: CH on two lanes per bus (codegen.row_pair_plan) -- the source of row 0, the source of row 1, the banks of CH
enum : int { ROW_PAR = 0, ROW_CH = 1, ROW_WS = 2, ROW_CH_PAIR = 3 };
template <class T, int W>
constexpr int row_src(int i, int hi) {
  return i >= hi ? -1 : (W == ROW_PAR ? T::T_ROW_PAR_SRC[i] : (W == ROW_CH ? T::T_ROW_CH_SRC[i] : (W == ROW_WS ? T::T_ROW_WS_SRC[i] : T::T_ROW2_CH_SRC0[i])));
}
template <class T, int W>
constexpr int row_src1(int i, int hi) {
  return (W != ROW_CH_PAIR || i >= hi) ? -1 : T::T_ROW2_CH_SRC1[i];
}
template <class T, int W>
constexpr int row_bank(int i, int hi) {
  return i >= hi ? 0 : (W == ROW_PAR ? T::T_ROW_PAR_BANK[i] : (W == ROW_WS ? T::T_ROW_WS_BANK[i] : T::T_ROW_CH_BANK[i]));
}
// the hand-overs [LO, HI) of table W, four to a statement: f(FIRST, N0, B0, ... N3, B3, M0, ... M3) with integral constants
// (FIRST: the point's first statement, the one that takes the lead)
#define ANM_ROW_PARAMS auto N0, auto B0, auto N1, auto B1, auto N2, auto B2, auto N3, auto B3, auto M0, auto M1, auto M2, auto M3
#define ANM_ROW_ARGS N0, B0, N1, B1, N2, B2, N3, B3, M0, M1, M2, M3
template <class T, int W, int LO, int HI, class F>
__device__ __forceinline__ void row_points(F&& f) {
  static_for<0, (HI - LO + 3) / 4>([&](auto Q) {
    constexpr int i = LO + 4 * int(Q);
#define ANM_ROW_IC(FN, k) std::integral_constant<int, FN<T, W>((k), HI)>{}
    f(std::bool_constant<int(Q) == 0>{}, ANM_ROW_IC(row_src, i), ANM_ROW_IC(row_bank, i), ANM_ROW_IC(row_src, i + 1),
      ANM_ROW_IC(row_bank, i + 1), ANM_ROW_IC(row_src, i + 2), ANM_ROW_IC(row_bank, i + 2), ANM_ROW_IC(row_src, i + 3),
      ANM_ROW_IC(row_bank, i + 3), ANM_ROW_IC(row_src1, i), ANM_ROW_IC(row_src1, i + 1), ANM_ROW_IC(row_src1, i + 2), ANM_ROW_IC(row_src1, i + 3));
#undef ANM_ROW_IC
  });
}

// LDS slot of one handed-over solve: 5 per-bus arrays + the iteration count / flags
template <class T>
struct Slot {
  static constexpr int VM = 0, CS = T::NB, SN = 2 * T::NB, P = 3 * T::NB, Q = 4 * T::NB, IT = 5 * T::NB,
                       FLAGS = IT + 1, SIZE = FLAGS + 1;
};

template <class T>
struct Shape {
  static constexpr int G = T::GRP;        // lanes per environment
  static constexpr int NG = 64 / G;       // environments per wavefront
};

// 2x2 inverse with ONE Newton step on v_rcp_f64 (measured on MI355X: rcp 24.4 bits, one step 48.7 bits = 2.2e-15
// relative, two steps 52.0 bits).  An inexact inverse perturbs a Newton STEP by that much and nothing else -- the
// fixed point is set by F, evaluated in full precision -- so the lane-group path, which only ever serves
// diverging solves and the rare 7- or 8-iteration ones, trades the second step for a shorter dependent chain;
// the thread-per-environment path keeps two steps (its iterates are pinned bit for bit by round-1 tests).
__device__ __forceinline__ Blk<double> blk_inv_fast(const Blk<double>& m) {
  const double det = fm(m.a, m.d, -(m.b * m.c));
  double r = __builtin_amdgcn_rcp(det);
  r = r * fma(-det, r, 2.0);
  return Blk<double>{m.d * r, -m.b * r, -m.c * r, m.a * r};
}
__device__ __forceinline__ Blk<float> blk_inv_fast(const Blk<float>& m) { return blk_inv(m); }

// What a lane knows about its place in the tree (constant tables indexed by the lane: loaded once).
template <class T>
struct LaneView {
  int l, gb, b;            // position in the group, first lane of the group, bus played (0: padding lane)
  bool lane_bus;
  int height, depth, nch;
  Lanes<T> X;
  double ybb_r, ybb_i, ybp_r, ybp_i, ypb_r, ypb_i;   // Y_bb, Y_b,parent, Y_parent,b (padding lanes: 0 -> W = 0)
  unsigned long long gmask; // lanes of my group
  unsigned pk[T::T_LP_NW > 0 ? T::T_LP_NW : 1];   // this lane's row of codegen.lane_pack (group-relative lanes)
  bool dpp_child;           // hybrid plan: the heavy child of this lane's bus sits in the next lane

  __device__ __forceinline__ void init() {
    constexpr int G = T::GRP;
    constexpr int PAD = first_padding_lane<T>();
    static_assert(PAD >= 0, "a lane group needs a padding lane (codegen.tree_tables)");
    const int lane = threadIdx.x & 63;
    l = lane & (G - 1);
    gb = lane - l;
    gmask = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << gb;
    ybb_r = ybb_i = ybp_r = ybp_i = ypb_r = ypb_i = 0.0;
    dpp_child = false;
    if constexpr (T::T_LP_NW > 0) {
      // ONE row of packed words per lane (a single vector load) instead of the chain lane -> bus -> parent -> lane of the
      // parent through three tables: three dependent loads in front of the first Newton trip of every wavefront
      static_for<0, T::T_LP_NW>([&](auto K) { pk[K] = T::T_LP[l * T::T_LP_NW + K]; });
      const unsigned w0 = pk[0];
      b = int(w0 & 0x7Fu);
      lane_bus = b > 0;
      height = int((w0 >> 7) & 0x7Fu) - 1;
      depth = int((w0 >> 14) & 0x7Fu) - 1;
      nch = int((w0 >> 21) & 0xFu);
      X.psrc4 = 4 * (gb + int((w0 >> 25) & 0x3Fu));
      dpp_child = (w0 >> 31) != 0u;
      static_for<0, T::T_MAXCH>([&](auto Cc) { X.csrc4[Cc] = 4 * (gb + int((pk[1 + Cc / 4] >> (8 * (Cc % 4))) & 0xFFu)); });
      return;
    }
    b = T::T_LANE_BUS[l];
    lane_bus = b > 0;
    const int parent = T::T_PARENT[b];               // 0: slack (b is a root of the elimination forest)
    height = lane_bus ? T::T_HEIGHT[b] : -1;
    depth = lane_bus ? T::T_DEPTH[b] : -1;
    nch = lane_bus ? T::T_NCH[b] : 0;
    X.psrc4 = 4 * (gb + ((lane_bus && parent > 0) ? T::T_POS[parent] : PAD));
    static_for<0, T::T_MAXCH>([&](auto Cc) {
      const int c = lane_bus ? T::T_CH[b * T::T_MAXCH + Cc] : -1;
      X.csrc4[Cc] = 4 * (gb + (c > 0 ? T::T_POS[c] : PAD));
    });
  }
  __device__ __forceinline__ void load_y(cptr_t C) {   // admittances of the compiled network
    typedef Layout<T> L;
    if (lane_bus) {
      ybb_r = C[L::Y_RE + T::T_ZBB[b]]; ybb_i = C[L::Y_IM + T::T_ZBB[b]];
      ybp_r = C[L::Y_RE + T::T_ZBP[b]]; ybp_i = C[L::Y_IM + T::T_ZBP[b]];
      ypb_r = C[L::Y_RE + T::T_ZPB[b]]; ypb_i = C[L::Y_IM + T::T_ZPB[b]];
    }
  }
};

// hybrid hand-overs: position of level h's first light-child slot in the packed list (sum of T_NLH below h)
template <class T>
constexpr int hyb_slot_base(int h) {
  int n = 0;
  for (int k = 0; k < h && k <= T::T_MAXH; ++k) n += T::T_NLH[k];
  return n;
}

// The update of the lanes of updm by the Newton step (d0: angle, d1: relative magnitude): rotation of (cos, sin) by d0, path
// chosen per wavefront exactly as update_angles does (the reduction of a small step returns the same bits as the short
// path).  The loops where a trip's instruction COUNT is its duration: the polynomials are evaluated on every lane -- a lane
// that does not update computes on whatever its d0 holds and drops the result -- so that the wave-uniform branch is the only
// control flow in front of them, and the rotation stands once behind both paths.
template <class JT>
__device__ __forceinline__ void update_iterate(unsigned long long updm, JT d0, JT d1, double& vm, double& cs, double& sn) {
  const bool upd = __builtin_amdgcn_inverse_ballot_w64(updm);
  const double dth = double(d0);
  const unsigned long long bigm = __builtin_amdgcn_fcmp(fabs(dth), 0.78, FCMP_UGT) & updm;  // NaN counts
  double sd_, cd_;
  if (bigm == 0ull) {
    sincos_kernel<true>(dth, 0, sd_, cd_);
  } else {
    sincos_medium<true>(dth, sd_, cd_);
    // (beyond the two-stage reduction: a handful of lanes per million solves -- the library routine then runs on every
    // lane of the wavefront and the lanes it was called for take its result: no divergent region in this tail)
    const bool ish = !(fabs(dth) < SINCOS_MEDIUM_MAX);
    if ((__builtin_amdgcn_uicmp(ish ? 1u : 0u, 0u, ICMP_NE) & updm) != 0ull) {
      const SinCos r = sincos_huge(dth);
      sd_ = ish ? r.s : sd_;
      cd_ = ish ? r.c : cd_;
    }
  }
  if (upd) {
    vm = fma(-double(d1), fabs(vm), vm);
    // (three-address v_fma_f64 in place of the compiler's v_fmac into a temporary + v_mov_b64 back into the loop's register)
    const double t1 = sn * sd_, t2 = cs * sd_;
    cs = fma3<false>(cs, cd_, t1);
    sn = fma3<true>(sn, cd_, t2);
  }
}

// The Newton-Raphson loop of every lane group of the wavefront, from the iterate (vm, cs, sn) each bus lane
// holds, `it` iterations already done.  gvalid (uniform per group): the group holds a solve.  Every lane of
// the wavefront must call.  On return: the final iterate, `it`, and the group's verdict in tb / tn
// (tb != 0: ||F||inf > tol or NaN; tn != 0: F has a NaN).
// LDSX (trees without a DPP plan; xl: 640 doubles private to the wavefront, 16-byte aligned): the hand-overs go
// through LDS -- a lane PUBLISHES what its parent (or its children) will need in its own slot, the consumer reads
// the slot of the lane it needs -- instead of ds_bpermute: a pair of doubles is one 16-byte write / read instead of
// four bpermutes, and the 5 child slots x 6 values of a bushy level cost 15 reads instead of 60 bpermutes.
// Padding lanes never publish; their slots hold the neutral values (zeroed here, V = 1).
// MERGED = false: the loop as it stood before the instruction-count cuts of round 6 (one region per fold, predicated child
// sums, no copies): 21 registers fewer -- what the radial kernel with per-group classes needs on a tree with a DPP plan to keep
// three wavefronts per SIMD.
template <class T, class JT, int EARLY_EXIT_TRIPS = 0, bool LDSX = false, int FETCH = LDSX_FETCH, bool WFREE = true, bool VPOLY = !LDSX,
          bool MERGED = true>
__device__ __forceinline__ void newton_groups(const LaneView<T>& V, bool gvalid, double& vm, double& cs, double& sn,
                                              double bus_p, double bus_q, int& it, unsigned& tb, unsigned& tn,
                                              double tol, int max_iter, double* xl = nullptr) {
  const Lanes<T>& X = V.X;
  static_assert(!LDSX || T::T_DPP == 0, "LDS hand-overs are the alternative to ds_bpermute, not to DPP moves");
  [[maybe_unused]] const int wl = threadIdx.x & 63;
  [[maybe_unused]] const int pl = X.psrc4 >> 2;                       // lane of the parent (or a padding lane)
  // LDS variant, back substitution without regions: every lane recomputes its step at every level -- from its own level on
  // its parent's step is final, so it recomputes the same value -- and a bus that hangs off the slack reads a step of zero:
  // the W slot of a padding lane (its admittances are zero), 64 slots behind the V slots.
  [[maybe_unused]] const int plb = V.depth == 0 ? 64 + pl : pl;
  [[maybe_unused]] int cl[T::T_MAXCH > 0 ? T::T_MAXCH : 1];           // lanes of the children (or a padding lane)
  static_for<0, T::T_MAXCH>([&](auto Cc) { cl[Cc] = X.csrc4[Cc] >> 2; });
  // LDS hand-overs: what a lane publishes sits TOGETHER in its slot -- (re, im) pairs and the six values a parent folds
  // as 16-byte units -- so that every access is a ds_read_b128 / ds_write_b128: four LDS cycles per wavefront
  // instruction where two 8-byte accesses 64 slots apart (ds_read2st64_b64, what separate arrays give) take eight.
  // The 12 wavefronts of a compute unit share ONE LDS pipe, and this loop keeps it busier than any VALU.
  //   xV[lane] = V (re, im), later the Newton step;  xW[lane] = W_pb;  xS[3 lane + 0 .. 2] = (Sc.a, Sc.b), (Sc.c, Sc.d), (Lr0, Lr1)
  [[maybe_unused]] double2* const xV = reinterpret_cast<double2*>(xl);
  [[maybe_unused]] double2* const xW = xV + 64;
  [[maybe_unused]] double2* const xS = xV + 128;
  if constexpr (LDSX) {
    xW[wl] = double2{0.0, 0.0};
    xS[3 * wl] = double2{0.0, 0.0}; xS[3 * wl + 1] = double2{0.0, 0.0}; xS[3 * wl + 2] = double2{0.0, 0.0};
    ANM_WAVE_SYNC();
  }
  // Hybrid hand-overs of the elimination (codegen.hybrid_plan; LDS variant only): the buses lie along their heavy edges, so
  // the child a bus's own elimination waits for -- the one of height h - 1 -- sits in the next lane and its six values
  // arrive by DPP (row_shl:1, no LDS round trip on the longest chain); every other child is folded through its LDS slot at
  // the level right after its own, by a parent that has nothing else to do then.  lq[h][j]: slot index (3 x lane) of the
  // j-th light child this lane's bus folds at level h (no such child: a padding lane's slot, zeros).
  constexpr bool HYB = LDSX && T::T_HYB != 0;
  // (the lanes of the children are per-lane constants of the whole loop: packed four to a register -- a byte each, one
  // v_bfe_u32 to take one out -- or they cost the kernel its third wavefront per SIMD: 170 registers instead of <= 168)
  constexpr int NLQ = HYB ? hyb_slot_base<T>(T::T_MAXH + 1) : 0;
  [[maybe_unused]] unsigned lqp[HYB ? (NLQ + 3) / 4 + 1 : 1] = {0u};
  [[maybe_unused]] unsigned clp[HYB ? (T::T_MAXCH + 3) / 4 : 1] = {0u};
  [[maybe_unused]] const bool dpp_child = V.dpp_child;   // this lane's bus has its heavy child in the next lane
  if constexpr (HYB) {
    static_assert(T::T_LP_NW > 0, "the hybrid plan comes with the packed lane table (codegen.lane_pack)");
    // (the table holds group-relative lanes, a byte each: + the first lane of the group in every byte)
    const unsigned gb1 = unsigned(V.gb) * 0x01010101u;
    static_for<0, (NLQ + 3) / 4>([&](auto K) { lqp[K] = V.pk[T::T_LP_LQ + K] + gb1; });
    static_for<0, (T::T_MAXCH + 3) / 4>([&](auto K) { clp[K] = V.pk[1 + K] + gb1; });
  }
  [[maybe_unused]] auto child_lane = [&](auto Cc) -> int {   // lane of the Cc-th child (W sums)
    if constexpr (HYB) return int(__builtin_amdgcn_ubfe(clp[Cc / 4], 8u * (Cc % 4), 8u));
    else return cl[Cc];
  };
  const int height = V.height, depth = V.depth, nch = V.nch;
  const double ybb_r = V.ybb_r, ybb_i = V.ybb_i, ybp_r = V.ybp_r, ybp_i = V.ybp_i, ypb_r = V.ypb_r, ypb_i = V.ypb_i;
  const unsigned long long gmask = V.gmask;
  const bool isbus = V.lane_bus && gvalid;
  {
    // ---- the reference's loop, rotated like pf_iterate (anm_device.hpp): evaluate; account for the update of
    // the previous trip; leave when no group runs; update.  `running` is uniform over a group; a group that
    // stopped (or holds no solve) rides along: its lanes keep executing, nothing of it changes any more.
    // Predicates live as 64-bit lane masks in scalar registers (v_cmp writes them there; the loop control is
    // then SALU work): `runm` = lanes of the groups that are still iterating.
    const unsigned long long busm = __builtin_amdgcn_uicmp(isbus ? 1u : 0u, 0u, ICMP_NE);
    unsigned long long runm = __builtin_amdgcn_uicmp(gvalid ? 1u : 0u, 0u, ICMP_NE);
    const unsigned glo = unsigned(gmask & busm), ghi = unsigned((gmask & busm) >> 32);   // bus lanes of my group
    tb = 0u; tn = 0u;
    it -= gvalid ? 1 : 0;        // the first trip only evaluates: its `it += running` is undone here
    // What a lane publishes for its parent (Schur complement, reduced right-hand side) and its Newton step:
    // a bus lane rewrites them at its own level of every trip before anybody reads them; a padding lane never
    // does, so these zeros are the neutral values the hand-overs rely on.
    Blk<JT> Sc = Blk<JT>{JT(0), JT(0), JT(0), JT(0)};
    JT Lr0 = JT(0), Lr1 = JT(0), d0 = JT(0), d1 = JT(0);
    constexpr bool ROOT_STEP_IN_PIVOT = !LDSX && T::T_LP_NW > 0 && MERGED;
    constexpr bool WSUM_FREE = WFREE && !LDSX && MERGED && T::T_MAXCH > 0 && child_moves_land_on_parents_or_zero<T>();
    constexpr bool WSUM_ONE = WSUM_FREE && child_moves_write_the_same_lanes<T>();
    [[maybe_unused]] double wr[T::T_MAXCH > 0 ? T::T_MAXCH : 1] = {0.0}, wi[T::T_MAXCH > 0 ? T::T_MAXCH : 1] = {0.0};
    [[maybe_unused]] int trip = 0;
    for (;;) {
      const double vr = vm * cs, vi = vm * sn;
      double vpr, vpi;
      if constexpr (LDSX) {
        xV[wl] = double2{vr, vi};
        ANM_WAVE_SYNC();
        const double2 vp = xV[pl];
        vpr = vp.x; vpi = vp.y;
      } else {
        vpr = X.from_parent(vr, 1.0); vpi = X.from_parent(vi, 0.0);
      }
      // W_bb = conj(Y_bb) vm^2;  P = V_b conj(V_p):  W_bp = conj(Y_bp) P,  W_pb = conj(Y_pb) conj(P)
      const double m2 = vm * vm;
      const double wbb_r = ybb_r * m2, wbb_i = -(ybb_i * m2);
      const double pr = fma(vr, vpr, vi * vpi), pim = fma(vi, vpr, -(vr * vpi));
      const double wbp_r = fma(ybp_r, pr, ybp_i * pim), wbp_i = fma(ybp_r, pim, -(ybp_i * pr));
      // (TRIM: the imaginary part is carried with its sign flipped -- the flip rides on the operands of its consumers instead of
      // being an instruction in front of the moves that hand it to the parent)
      constexpr bool TRIM = MERGED;   // (the LDS variant too: what it publishes is the unflipped value)
      const double wpb_r = fma(ypb_r, pr, -(ypb_i * pim)), nwpb_i = fma(ypb_r, pim, ypb_i * pr);
      [[maybe_unused]] const double wpb_i = -nwpb_i;
      // S_b = W_bb + W_bp + sum over the children c of W_pb(c)
      double sr = wbb_r + wbp_r, si = wbb_i + wbp_i;
      if constexpr (LDSX) {
        xW[wl] = TRIM ? double2{wpb_r, nwpb_i} : double2{wpb_r, wpb_i};
        ANM_WAVE_SYNC();
      }
      if constexpr (WSUM_FREE) {
        // (no predicate: see child_moves_land_on_parents_or_zero; wr / wi are loop-carried so that the lanes no move writes
        // keep their zeros)
        static_for<0, T::T_MAXCH>([&](auto Cc) {
          constexpr int K = WSUM_ONE ? 0 : int(Cc);   // (all classes write the same lanes: one register receives them in turn)
          wr[K] = dpp_move<T::T_CH_CTRL[2 * Cc], T::T_CH_BANK[2 * Cc], 0, false>(wr[K], wpb_r);
          wi[K] = dpp_move<T::T_CH_CTRL[2 * Cc], T::T_CH_BANK[2 * Cc], 0, false>(wi[K], nwpb_i);
          sr += wr[K];
          si -= wi[K];
        });
      } else
      static_for<0, T::T_MAXCH>([&](auto Cc) {
        double cr, ci;
        if constexpr (LDSX) {
          const double2 cw = xW[child_lane(Cc)];
          cr = cw.x; ci = cw.y;
        } else {
          cr = X.template from_child<Cc>(wpb_r); ci = X.template from_child<Cc>(TRIM ? nwpb_i : wpb_i);
        }
        if (Lanes<T>::template child_neutral<Cc>() || Cc < nch) {
          sr += cr;
          if constexpr (TRIM) si -= ci; else si += ci;
        }
      });
      const double fr = sr - bus_p, fi = si - bus_q;
      // group-wide stop test: "||F||inf > tol" and "F has a NaN" are all the reference's loop and flags need.
      // A group that has stopped keeps evaluating the same frozen iterate, so what the last trip computed
      // is also each group's final verdict: nothing but `runm` and `it` is carried over.  (The verdict OR-ed over the group
      // by a butterfly of DPP-operand v_or_b32 instead: headline kernel 74.7 -> 79.2 us, same box -- it sits on the exit chain.)
      const unsigned long long badm = __builtin_amdgcn_fcmp(fmax(fabs(fr), fabs(fi)), tol, FCMP_UGT);
      const unsigned long long nanm = __builtin_amdgcn_fcmp(fr, fi, FCMP_UNO);
      tb = (unsigned(badm) & glo) | (unsigned(badm >> 32) & ghi);
      tn = (unsigned(nanm) & glo) | (unsigned(nanm >> 32) & ghi);
      it += __builtin_amdgcn_inverse_ballot_w64(runm) ? 1 : 0;   // the update applied in the previous trip
      runm &= __builtin_amdgcn_uicmp(tb, 0u, ICMP_NE) & ~__builtin_amdgcn_uicmp(tn, 0u, ICMP_NE) &
              __builtin_amdgcn_sicmp(it, max_iter, ICMP_SLT);   // NaN > tol is false, like the reference
      // The loop is left at the END of the trip: the scalar chain compare -> masks -> branch then overlaps the
      // elimination instead of stalling the wavefront in front of it every trip (what counts for the ~94 trips
      // of a diverging solve); the price is one idle elimination when the last group stops (its update is
      // masked: `runm` is 0).  A caller whose whole batch passes through here (anm_radial.hpp: four or five
      // trips per solve, so an idle elimination is one trip in five) asks for the branch to be taken on the
      // spot during the first EARLY_EXIT_TRIPS trips.
      const bool all_done = runm == 0ull;
      if constexpr (EARLY_EXIT_TRIPS > 0) {
        if (all_done && trip < EARLY_EXIT_TRIPS) break;
        ++trip;
      }

      // ---- Jacobian blocks (anm_device.hpp: newton_update): own diagonal and the two couplings with the parent
      // (TRIM: wbb_i - si for -(si - wbb_i): one subtraction, not a subtraction and a sign flip of a value that is then
      // updated in place; the two differ in the sign of a zero)
      Blk<JT> Dg = Blk<JT>{TRIM ? JT(wbb_i - si) : JT(-(si - wbb_i)), JT(sr + wbb_r), JT(sr - wbb_r), JT(si + wbb_i)};
      const Blk<JT> Jbp = Blk<JT>{JT(wbp_i), JT(wbp_r), JT(-wbp_r), JT(wbp_i)};
      const Blk<JT> Jpb = TRIM ? Blk<JT>{JT(-nwpb_i), JT(wpb_r), JT(-wpb_r), JT(-nwpb_i)}
                               : Blk<JT>{JT(wpb_i), JT(wpb_r), JT(-wpb_r), JT(wpb_i)};
      JT r0 = JT(fr), r1 = JT(fi);
      // ---- elimination by height: a bus folds the Schur complements and reduced right-hand sides its
      // children published (registers Sc / Lr of the child lanes; 0 on padding lanes), inverts its pivot
      // and publishes its own
      if constexpr (HYB) {
        // (`height` captured first, by value: the register assignment the compiler makes follows the closure's layout, and this
        // one gives the code that was measured)
        static_for<0, T::T_MAXH + 1>([&, height](auto H) {
          constexpr int h = H;
          if constexpr (h > 0) {
            constexpr int NL = T::T_NLH[h];
            // light children of height h - 1 (published at the end of the previous level), folded by every bus that has some --
            // whatever its own height -- one slot at a time (two fetched together: 170 registers, the third wavefront per SIMD
            // lost).  Every lane reads and folds: a lane without such a child reads a padding lane's slot, zeros, also after its
            // own pivot -- no region around the reads.
            static_for<0, NL>([&](auto Q) {
              constexpr int q = hyb_slot_base<T>(h) + Q;
              const int cq = 3 * int(__builtin_amdgcn_ubfe(lqp[q / 4], 8u * (q % 4), 8u));
              const double2 q0 = xS[cq], q1 = xS[cq + 1], q2 = xS[cq + 2];
              __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): ONE wait for the slot's three reads (else one per 16-byte unit)
              Dg.a -= JT(q0.x); Dg.b -= JT(q0.y); Dg.c -= JT(q1.x); Dg.d -= JT(q1.y);
              r0 -= JT(q2.x); r1 -= JT(q2.y);
            });
            // the heavy child's publication: registers of the next lane (every lane executes the moves; only the buses of
            // this height, whose next lane IS their child of height h - 1, use what arrives)
            constexpr int SHL1 = 0x101;   // row_shl:1 -- lane i reads lane i + 1 of its 16-lane row
            const JT ha = dpp_move<SHL1, 0xF, 1, true>(JT(0), Sc.a), hb = dpp_move<SHL1, 0xF, 1, true>(JT(0), Sc.b);
            const JT hc = dpp_move<SHL1, 0xF, 1, true>(JT(0), Sc.c), hd = dpp_move<SHL1, 0xF, 1, true>(JT(0), Sc.d);
            const JT h0 = dpp_move<SHL1, 0xF, 1, true>(JT(0), Lr0), h1 = dpp_move<SHL1, 0xF, 1, true>(JT(0), Lr1);
            if (height == h && (T::T_ALL_HEAVY != 0 || dpp_child)) {
              Dg.a -= ha; Dg.b -= hb; Dg.c -= hc; Dg.d -= hd;
              r0 -= h0; r1 -= h1;
            }
          }
          if (height == h) {
            Dg = blk_inv_fast(Dg);
            if constexpr (h < T::T_MAXH) {
              const Blk<JT> Lk = blk_mul(Jpb, Dg);
              Sc = blk_mul(Lk, Jbp);
              Lr0 = fm(Lk.a, r0, Lk.b * r1);
              Lr1 = fm(Lk.c, r0, Lk.d * r1);
              xS[3 * wl] = double2{double(Sc.a), double(Sc.b)};
              xS[3 * wl + 1] = double2{double(Sc.c), double(Sc.d)};
              xS[3 * wl + 2] = double2{double(Lr0), double(Lr1)};
            }
          }
          if constexpr (h < T::T_MAXH) ANM_WAVE_SYNC();
        });
      } else if constexpr (!LDSX && T::T_LP_NW > 0 && MERGED) {
        // Register hand-overs, every child folded at the level right after its OWN (see the next variant), with the
        // predicated code of a level gathered: all moves of the level first (every lane executes them), then ONE region
        // for the buses of this height -- their folds (no predicate of its own for a child class every bus of this height
        // folds now: the 6-bus feeder's only kind) and the pivot -- and one per child class a HIGHER bus folds early.  Each
        // region the compiler opens is a save / restore pair of the exec mask (+ a skip branch for a long one): issue
        // slots like any other for a wavefront that iterates alone on its SIMD.  Same operations on every bus, in the
        // same order: bit-identical to the one-region-per-fold form (MERGED = false).
        // Level 0 has nothing to fold, so its pivot needs no region either when it writes to a copy (Di) and no leaf hangs
        // off the slack: every lane computes it, a bus of a greater height (and a padding lane) on an unfinished block --
        // what that publishes is rewritten at the bus's own level before its parent reads it, a padding lane's is read by nobody.
        constexpr bool L0_FREE = roots_at_height<T>(0) == 0;
        Blk<JT> Di = Dg;   // (a padding lane's copy stays as it is: nobody reads it)
        static_for<0, T::T_MAXH + 1>([&](auto H) {
          constexpr int h = H;
          [[maybe_unused]] JT g[T::T_MAXCH][6];
          [[maybe_unused]] auto mine_now = [&](auto Cc) {   // my Cc-th child has height h - 1
            return ((V.pk[T::T_LP_HH + Cc / 4] >> (8 * (Cc % 4))) & 0xFFu) == unsigned(h);
          };
          [[maybe_unused]] auto fold = [&](auto Cc) {
            Dg.a -= g[Cc][0]; Dg.b -= g[Cc][1]; Dg.c -= g[Cc][2]; Dg.d -= g[Cc][3];
            r0 -= g[Cc][4]; r1 -= g[Cc][5];
          };
          if constexpr (h > 0) {
            static_for<0, T::T_MAXCH>([&](auto Cc) {
              if constexpr (T::T_CLS_H[h * T::T_MAXCH + Cc] != 0) {
                g[Cc][0] = X.template from_child<Cc>(Sc.a); g[Cc][1] = X.template from_child<Cc>(Sc.b);
                g[Cc][2] = X.template from_child<Cc>(Sc.c); g[Cc][3] = X.template from_child<Cc>(Sc.d);
                g[Cc][4] = X.template from_child<Cc>(Lr0); g[Cc][5] = X.template from_child<Cc>(Lr1);
              }
            });
          }
          const bool at_level = (h == 0 && L0_FREE) ? true : (height == h);   // (a constant at a free level 0: no region)
          if (at_level) {
            if constexpr (h > 0) {
              static_for<0, T::T_MAXCH>([&](auto Cc) {
                if constexpr (fold_at_own_level<T>(h, Cc) == 2) fold(Cc);
                else if constexpr (fold_at_own_level<T>(h, Cc) == 1) { if (mine_now(Cc)) fold(Cc); }
              });
            }
            Di = blk_inv_fast(Dg);
            // (the Newton step of a bus that hangs off the slack -- the first level of the back substitution -- right here,
            // inside the region of its pivot: the same expression, no region or select of its own)
            if constexpr (roots_at_height<T>(h) == 2) {
              d0 = fm(Di.a, r0, Di.b * r1);
              d1 = fm(Di.c, r0, Di.d * r1);
            } else if constexpr (roots_at_height<T>(h) == 1) {
              if (depth == 0) {
                d0 = fm(Di.a, r0, Di.b * r1);
                d1 = fm(Di.c, r0, Di.d * r1);
              }
            }
            if constexpr (h < T::T_MAXH) {
              const Blk<JT> Lk = blk_mul(Jpb, Di);
              Sc = blk_mul(Lk, Jbp);
              Lr0 = fm(Lk.a, r0, Lk.b * r1);
              Lr1 = fm(Lk.c, r0, Lk.d * r1);
            }
          }
          if constexpr (h > 0) {
            static_for<0, T::T_MAXCH>([&](auto Cc) {
              if constexpr (fold_early<T>(h, Cc)) { if (height > h && mine_now(Cc)) fold(Cc); }
            });
          }
        });
        Dg = Di;   // (the back substitution reads the inverted pivots from Dg)
      } else if constexpr (!LDSX && T::T_LP_NW > 0) {
        // Register hand-overs (DPP moves / ds_bpermute), every child folded at the level right after its OWN (whatever the
        // height of its parent: a parent of a higher level has nothing else to do then) -- a level moves only the child
        // classes some bus really folds there (T_CLS_H): the 6-bus feeder moves 2 + 1 classes instead of 2 + 2, twelve to
        // twenty-four DPP moves of a 375-instruction trip.  (height + 1 of each child of this lane's bus: a byte each in the packed row)
        static_for<0, T::T_MAXH + 1>([&](auto H) {
          constexpr int h = H;
          if constexpr (h > 0) {
            static_for<0, T::T_MAXCH>([&](auto Cc) {
              if constexpr (T::T_CLS_H[h * T::T_MAXCH + Cc] != 0) {
                const JT ga = X.template from_child<Cc>(Sc.a), gbb = X.template from_child<Cc>(Sc.b);
                const JT gc = X.template from_child<Cc>(Sc.c), gd = X.template from_child<Cc>(Sc.d);
                const JT g0 = X.template from_child<Cc>(Lr0), g1 = X.template from_child<Cc>(Lr1);
                if (((V.pk[T::T_LP_HH + Cc / 4] >> (8 * (Cc % 4))) & 0xFFu) == unsigned(h)) {   // my Cc-th child has height h - 1
                  Dg.a -= ga; Dg.b -= gbb; Dg.c -= gc; Dg.d -= gd;
                  r0 -= g0; r1 -= g1;
                }
              }
            });
          }
          if (height == h) {
            Dg = blk_inv_fast(Dg);
            if constexpr (h < T::T_MAXH) {
              const Blk<JT> Lk = blk_mul(Jpb, Dg);
              Sc = blk_mul(Lk, Jbp);
              Lr0 = fm(Lk.a, r0, Lk.b * r1);
              Lr1 = fm(Lk.c, r0, Lk.d * r1);
            }
          }
        });
      } else
      static_for<0, T::T_MAXH + 1>([&](auto H) {
        constexpr int h = H;
        constexpr int NC = T::T_NCH_H[h];
        // register hand-overs: every lane executes the moves, so they are collected first (NC child slots x 6
        // values); LDS hand-overs: only the lanes of this height read, and fold as they read -- no staging arrays
        // (they cost the LDS variant 9 registers too many for a third wavefront per SIMD)
        JT ga[(!LDSX && NC > 0) ? NC : 1], gbb[(!LDSX && NC > 0) ? NC : 1], gc[(!LDSX && NC > 0) ? NC : 1],
            gd[(!LDSX && NC > 0) ? NC : 1], g0[(!LDSX && NC > 0) ? NC : 1], g1[(!LDSX && NC > 0) ? NC : 1];
        if constexpr (!LDSX) {
          static_for<0, NC>([&](auto Cc) {
            ga[Cc] = X.template from_child<Cc>(Sc.a); gbb[Cc] = X.template from_child<Cc>(Sc.b);
            gc[Cc] = X.template from_child<Cc>(Sc.c); gd[Cc] = X.template from_child<Cc>(Sc.d);
            g0[Cc] = X.template from_child<Cc>(Lr0); g1[Cc] = X.template from_child<Cc>(Lr1);
          });
        }
        if (height == h) {
          static_for<0, NC>([&](auto Cc) {
            if constexpr (LDSX) {
              // FETCH (3; 2 where the caller is short of registers) child slots are fetched together, then folded (a padding lane's slots hold zeros):
              // staging all NC slots costs up to 60 registers (and the third wavefront per SIMD), one slot at a time one
              // LDS latency per child
              constexpr int F = FETCH;
              if constexpr (Cc % F == 0) {
                constexpr int NF = (NC - Cc) < F ? (NC - Cc) : F;   // slots of this round
                double2 qv[NF][3];
                static_for<0, NF>([&](auto Q) {
                  const int cq = 3 * cl[Cc + Q];
                  qv[Q][0] = xS[cq]; qv[Q][1] = xS[cq + 1]; qv[Q][2] = xS[cq + 2];
                });
                static_for<0, NF>([&](auto Q) {
                  Dg.a -= JT(qv[Q][0].x); Dg.b -= JT(qv[Q][0].y); Dg.c -= JT(qv[Q][1].x); Dg.d -= JT(qv[Q][1].y);
                  r0 -= JT(qv[Q][2].x); r1 -= JT(qv[Q][2].y);
                });
              }
            } else if (Lanes<T>::template child_neutral<Cc>() || Cc < nch) {
              Dg.a -= ga[Cc]; Dg.b -= gbb[Cc]; Dg.c -= gc[Cc]; Dg.d -= gd[Cc];
              r0 -= g0[Cc]; r1 -= g1[Cc];
            }
          });
          Dg = blk_inv_fast(Dg);
          if constexpr (h < T::T_MAXH) {  // a bus of maximal height hangs off the slack: nobody folds it
            const Blk<JT> Lk = blk_mul(Jpb, Dg);
            Sc = blk_mul(Lk, Jbp);
            Lr0 = fm(Lk.a, r0, Lk.b * r1);
            Lr1 = fm(Lk.c, r0, Lk.d * r1);
            if constexpr (LDSX) {
              xS[3 * wl] = double2{double(Sc.a), double(Sc.b)};
              xS[3 * wl + 1] = double2{double(Sc.c), double(Sc.d)};
              xS[3 * wl + 2] = double2{double(Lr0), double(Lr1)};
            }
          }
        }
        if constexpr (LDSX && h < T::T_MAXH) ANM_WAVE_SYNC();
      });
      // ---- back substitution by depth (Dg now holds the inverted pivots)
      static_for<0, T::T_MAXD + 1>([&](auto Dd) {
        constexpr int dd = Dd;
        JT p0 = JT(0), p1 = JT(0);
        if constexpr (dd > 0) {
          if constexpr (LDSX) {
            const double2 dp = xV[plb];
            p0 = JT(dp.x); p1 = JT(dp.y);
          } else {
            p0 = X.from_parent(d0, JT(0));
            p1 = X.from_parent(d1, JT(0));
          }
        }
        if constexpr (!(ROOT_STEP_IN_PIVOT && dd == 0))
        if (LDSX || depth == dd) {
          JT a0 = r0, a1 = r1;
          if constexpr (dd > 0) {
            a0 = fm(-Jbp.b, p1, fm(-Jbp.a, p0, a0));
            a1 = fm(-Jbp.d, p1, fm(-Jbp.c, p0, a1));
          }
          d0 = fm(Dg.a, a0, Dg.b * a1);
          d1 = fm(Dg.c, a0, Dg.d * a1);
          if constexpr (LDSX && dd < T::T_MAXD) xV[wl] = double2{double(d0), double(d1)};
        }
        if constexpr (LDSX && dd < T::T_MAXD) ANM_WAVE_SYNC();
      });
      // ---- update of the running groups; d1 is the relative magnitude step.  Rotation of (cos, sin) by the
      // angle step, path chosen per wavefront exactly as update_angles does (the reduction of a small step
      // returns the same bits as the short path)
      // (a padding lane's step is zero -- it never writes d0 / d1 -- and a rotation by zero returns its V = 1 bit for bit:
      // where the pads ride along, `& busm` is an instruction saved)
      const unsigned long long updm = (TRIM && !LDSX) ? runm : (runm & busm);
      const bool upd = __builtin_amdgcn_inverse_ballot_w64(updm);
      const double dth = double(d0);
      const unsigned long long bigm = __builtin_amdgcn_fcmp(fabs(dth), 0.78, FCMP_UGT) & updm;  // NaN counts
      if constexpr (VPOLY) {
        // (the register hand-over variant = the continuation of the thread family's diverging solves, and the LDS variant where the
        // caller's register budget has room for the coefficients in vector registers: the radial kernel without per-group classes, 163 of 168)
        update_iterate(updm, d0, d1, vm, cs, sn);
      } else
      if (bigm == 0ull) {
        if (upd) {
          double sd_, cd_;
          // (one-instruction Horner steps with the coefficients in vector registers -- see sincos_kernel -- where there is room: the
          // LDS-hand-over variant, which serves the radial kernel's larger trees, sits at its 168-register budget for three
          // wavefronts per SIMD and keeps the compiler's own form)
          sincos_kernel<!LDSX>(dth, 0, sd_, cd_);
          vm = fma(-double(d1), fabs(vm), vm);
          const double c0 = cs, s0 = sn;
          cs = fma(c0, cd_, s0 * sd_);
          sn = fma(s0, cd_, -(c0 * sd_));
        }
      } else if (upd) {
        double sd_, cd_;
        if (fabs(dth) < SINCOS_MEDIUM_MAX) {
          sincos_medium<!LDSX>(dth, sd_, cd_);
        } else {
          const SinCos r = sincos_huge(dth);
          sd_ = r.s;
          cd_ = r.c;
        }
        vm = fma(-double(d1), fabs(vm), vm);
        const double c0 = cs, s0 = sn;
        cs = fma(c0, cd_, s0 * sd_);
        sn = fma(s0, cd_, -(c0 * sd_));
      }
      if (all_done) break;
    }

  }
}

// The LDS hand-over of one solve between its owner lane (which holds the whole iterate) and the bus lanes that continue
// it, through the solve's slot s.  Four phases; the callers put a wavefront barrier behind each:
//   slot_send     the owner writes the iterate, the injections and the iteration count
//   slot_load     the lane of bus b reads its bus (every lane of a slot that holds a solve reads the count besides)
//   slot_store    the lane of bus b writes its iterate back, the lane of bus 1 also the count and the verdict of tb / tn
//                 (NaN: failed; 0: converged; +inf: still above tol)
//   slot_receive  the owner takes the final iterate, st.it and the verdict as st.diff
template <class T>
__device__ __forceinline__ void slot_send(double* s, const EnvWork<T>& w, const PFState<T>& st) {
  typedef Slot<T> S;
  static_for<1, T::NB>([&](auto I) {
    constexpr int i = I;
    s[S::VM + i] = w.vm[i]; s[S::CS + i] = st.cs[i]; s[S::SN + i] = st.sn[i];
    s[S::P + i] = w.bus_p[i]; s[S::Q + i] = w.bus_q[i];
  });
  s[S::IT] = double(st.it);
}
template <class T>
__device__ __forceinline__ void slot_load(const double* s, int b, double& vm, double& cs, double& sn, double& bus_p, double& bus_q) {
  typedef Slot<T> S;
  vm = s[S::VM + b]; cs = s[S::CS + b]; sn = s[S::SN + b]; bus_p = s[S::P + b]; bus_q = s[S::Q + b];
}
template <class T>
__device__ __forceinline__ void slot_store(double* s, int b, const double& vm, const double& cs, const double& sn, const int& it,
                                           const unsigned& tb, const unsigned& tn) {
  typedef Slot<T> S;
  s[S::VM + b] = vm; s[S::CS + b] = cs; s[S::SN + b] = sn;
  if (b == 1) {
    s[S::IT] = double(it);
    s[S::FLAGS] = (tn != 0u) ? NAN : ((tb != 0u) ? INFINITY : 0.0);
  }
}
template <class T>
__device__ __forceinline__ void slot_receive(const double* s, EnvWork<T>& w, PFState<T>& st) {
  typedef Slot<T> S;
  static_for<1, T::NB>([&](auto I) {
    constexpr int i = I;
    w.vm[i] = s[S::VM + i]; st.cs[i] = s[S::CS + i]; st.sn[i] = s[S::SN + i];
    w.vr[i] = w.vm[i] * st.cs[i];   // the iterate's V, as eval_mismatch leaves it (pf_end reads it)
    w.vi[i] = w.vm[i] * st.sn[i];
  });
  st.it = int(s[S::IT]);
  st.diff = s[S::FLAGS];
}

// Continue the Newton-Raphson solves of the lanes with st.active (they have done st.it iterations and
// hold their iterate in w.vm / st.cs / st.sn) until each converges, fails (NaN) or reaches max_iter --
// NG solves at a time, one per lane group.  On return the owner lanes hold the final iterate, st.it and
// a st.diff that reproduces the reference's flags (NaN: failed; 0: converged; +inf: cap reached).
// `lds`: >= NG * Slot<T>::SIZE doubles, private to this wavefront; every lane of the wave must call.
// WFREE = false: the predicate-free child sums (four to eight loop-carried registers) left out -- the straggler launch, whose
// budget is two wavefronts per SIMD.
// keep (max_iter below the caller's real cap, see continue_collective): a solve that stops only because it reached max_iter
// stays st.active with its iterate and count.
template <class T, class JT, bool WFREE = true>
__device__ __forceinline__ void continue_in_groups(cptr_t C, EnvWork<T>& w, PFState<T>& st, bool mine, double tol, int max_iter,
                                   double* lds, bool keep = false) {
  typedef Slot<T> S;
  constexpr int G = Shape<T>::G, NG = Shape<T>::NG;
  const int lane = threadIdx.x & 63;
  const int grp = lane / G;
  LaneView<T> V;
  V.init();
  V.load_y(C);
  const int b = V.b;

  // ---- which lanes hand over, in lane order; NG at a time
  const unsigned long long todo = __ballot(mine);
  const int n_todo = __popcll(todo);
  const int rank = __popcll(todo & ((1ull << lane) - 1ull));
  for (int base = 0; base < n_todo; base += NG) {
    const bool send = mine && rank >= base && rank < base + NG;
    if (send) slot_send<T>(lds + (rank - base) * S::SIZE, w, st);
    ANM_WAVE_SYNC();
    const bool gvalid = base + grp < n_todo;           // this group holds a solve
    const bool isbus = V.lane_bus && gvalid;
    double vm = 1.0, cs = 1.0, sn = 0.0, bus_p = 0.0, bus_q = 0.0;
    int it = 0;
    if (isbus) slot_load<T>(lds + grp * S::SIZE, b, vm, cs, sn, bus_p, bus_q);
    if (gvalid) it = int(lds[grp * S::SIZE + S::IT]);
    ANM_WAVE_SYNC();
    unsigned tb, tn;
    newton_groups<T, JT, 0, false, LDSX_FETCH, WFREE>(V, gvalid, vm, cs, sn, bus_p, bus_q, it, tb, tn, tol, max_iter);

    // ---- results back to the owner lanes
    if (isbus) slot_store<T>(lds + grp * S::SIZE, b, vm, cs, sn, it, tb, tn);
    ANM_WAVE_SYNC();
    if (send) {
      slot_receive<T>(lds + (rank - base) * S::SIZE, w, st);
      st.active = keep && st.diff == INFINITY;
    }
    ANM_WAVE_SYNC();
  }
}

// ---------------------------------------------------------------------------------------------
// One solve per 16-lane row (topologies with a codegen.row_plan): four solves per wavefront, one lane per bus, every
// hand-over of the trip one row_newbcast instruction (row_mov / row_wsum / row_fold / row_fma above).  The per-lane algebra
// is that of newton_groups<MERGED>: every floating-point operation of every bus is the same operation on the same
// operands in the same order -- only where an operand comes from changes -- so a solve gives the same bits on rows as on
// groups.  Nobody relies on neutral values in the unused lanes: every consumer names its source.
// ---------------------------------------------------------------------------------------------
template <class T>
struct RowView {
  int b;                   // bus played (0: unused lane)
  bool lane_bus;
  bool rep;                // two lanes per bus (codegen.row_pair_plan): this lane is replica 1 of its bus
  int height, depth;
  double ybb_r, ybb_i, ybp_r, ybp_i, ypb_r, ypb_i;   // Y_bb, Y_b,parent, Y_parent,b (unused lanes: 0)
  unsigned long long rmask; // lanes of my row

  __device__ __forceinline__ void init(cptr_t C, bool pairs = false) {
    typedef Layout<T> L;
    const int lane = threadIdx.x & 63;
    const unsigned w0 = pairs ? T::T_ROW2_LP[lane & 15] : T::T_ROW_LP[lane & 15];
    b = int(w0 & 0x7Fu);
    lane_bus = b > 0;
    rep = ((w0 >> 21) & 1u) != 0u;
    height = int((w0 >> 7) & 0x7Fu) - 1;
    depth = int((w0 >> 14) & 0x7Fu) - 1;
    rmask = 0xFFFFull << (lane & 48);
    ybb_r = ybb_i = ybp_r = ybp_i = ypb_r = ypb_i = 0.0;
    if (lane_bus) {
      ybb_r = C[L::Y_RE + T::T_ZBB[b]]; ybb_i = C[L::Y_IM + T::T_ZBB[b]];
      ybp_r = C[L::Y_RE + T::T_ZBP[b]]; ybp_i = C[L::Y_IM + T::T_ZBP[b]];
      ypb_r = C[L::Y_RE + T::T_ZPB[b]]; ypb_i = C[L::Y_IM + T::T_ZPB[b]];
    }
  }
};

// The sign of x flipped on the lanes whose `flip` holds the sign bit (0 elsewhere): one v_xor_b32 on the high word.
__device__ __forceinline__ double row_flip(double x, unsigned flip) {
  return __hiloint2double(__double2hiint(x) ^ int(flip), __double2loint(x));
}
__device__ __forceinline__ float row_flip(float x, unsigned flip) { return __uint_as_float(__float_as_uint(x) ^ flip); }

// newton_groups with rows for groups: same arguments, same results (rvalid: the row holds a solve, uniform per row).
// PAIRS: TWO lanes per bus (codegen.row_pair_plan; V initialised for pairs).  Both lanes of a bus are full replicas -- the
// same loads, W products, Dg, Di, step and update, so nothing ever moves between them, and they hold identical F, so every
// ballot says what it says with one lane per bus -- except that each forms ONE row of Lk = Jpb Di, Sc = Lk Jbp and Lr = Lk r:
// replica 0 row 0, replica 1 row 1, by the source expressions of blk_mul and of the one-lane form's Lr0 / Lr1 restricted to
// that row.  A fold names replica 0 of the child for Sc.a, Sc.b and Lr0 and replica 1 for Sc.c, Sc.d and Lr1
// (row_pair_fold); every other hand-over names replica 0.  Every floating-point operation that reaches a result is that of
// one lane per bus on the same operands in the same order: the same bits.  PAIRS guards three places: my row of Jpb, the
// products behind the pivot, the fold statement.
template <class T, class JT, bool PAIRS = false>
__device__ __forceinline__ void newton_rows(const RowView<T>& V, bool rvalid, double& vm, double& cs, double& sn, double bus_p,
                                            double bus_q, int& it, unsigned& tb, unsigned& tn, double tol, int max_iter) {
  static_assert(T::T_ROW != 0, "codegen.row_plan: the topology has no row layout");
  static_assert(!PAIRS || T::T_ROW2 != 0, "codegen.row_pair_plan: the topology has no row layout with two lanes per bus");
  const double ybb_r = V.ybb_r, ybb_i = V.ybb_i, ybp_r = V.ybp_r, ybp_i = V.ybp_i, ypb_r = V.ypb_r, ypb_i = V.ypb_i;
  const bool isbus = V.lane_bus && rvalid;
  const unsigned long long busm = __builtin_amdgcn_uicmp(isbus ? 1u : 0u, 0u, ICMP_NE);
  // The running lanes are the BUS lanes of the running rows: every lane computes every level's pivot and every depth's step
  // (below), so an unused lane carries Inf / NaN in its step (a zero pivot inverted).  Every ballot of the loop is taken
  // under runm or glo / ghi, both subsets of busm, the update is applied under runm, and the caller reads bus lanes only:
  // what an unused lane holds reaches no decision and no result.
  unsigned long long runm = busm;
  const unsigned glo = unsigned(V.rmask & busm), ghi = unsigned((V.rmask & busm) >> 32);   // bus lanes of my row
  [[maybe_unused]] const bool rep = V.rep;                          // (PAIRS: this lane forms row 1)
  [[maybe_unused]] const unsigned flip = rep ? 0x80000000u : 0u;
  tb = 0u; tn = 0u;
  it -= rvalid ? 1 : 0;        // the first trip only evaluates: its `it += running` is undone here
  // the voltage of the parent: a bus attached to the slack keeps 1 + 0j, every other bus receives its parent's every trip
  double vpr = 1.0, vpi = 0.0;
  // 1.0 in registers of its own for the fused folds (opaque to the compiler: not rematerialised in front of every use)
  double one = 1.0;
  asm volatile("" : "+v"(one));
  const JT onej = JT(one);
  // the loads issued before the loop (the caller's LDS reads, the admittances) are waited for HERE: left to the compiler,
  // their counters are waited for inside the loop, on every trip
  __builtin_amdgcn_s_waitcnt(0);
  for (;;) {
    // V = vm (cs + j sn) and vm^2 lead the hand-over of the parent's voltage (a tree without one: plain)
    double vr, vi, m2;
    if constexpr (T::T_ROW_PAR_N == 0) {
      vr = vm * cs; vi = vm * sn; m2 = vm * vm;
    } else {
      row_points<T, ROW_PAR, 0, T::T_ROW_PAR_N>([&](auto FIRST, ANM_ROW_PARAMS) {
        if constexpr (FIRST) row_mov_lead<ANM_ROW_ARGS>(vpr, vpi, vr, vi, m2, vm, cs, sn);
        else row_mov<ANM_ROW_ARGS>(vpr, vpi, vr, vi);
      });
    }
    // W_bb = conj(Y_bb) vm^2;  P = V_b conj(V_p):  W_bp = conj(Y_bp) P,  W_pb = conj(Y_pb) conj(P)
    const double wbb_r = ybb_r * m2, wbb_i = -(ybb_i * m2);
    const double pr = fma(vr, vpr, vi * vpi), pim = fma(vi, vpr, -(vr * vpi));
    const double wbp_r = fma(ybp_r, pr, ybp_i * pim), wbp_i = fma(ybp_r, pim, -(ybp_i * pr));
    const double wpb_r = fma(ypb_r, pr, -(ypb_i * pim)), nwpb_i = fma(ypb_r, pim, ypb_i * pr);   // (imaginary part: sign flipped)
    // S_b = W_bb + W_bp + sum over the children c of W_pb(c)
    double sr, si;
    if constexpr (T::T_ROW_CH_N == 0) {
      sr = wbb_r + wbp_r; si = wbb_i + wbp_i;
    } else {
      row_points<T, ROW_WS, 0, T::T_ROW_CH_N>([&](auto FIRST, ANM_ROW_PARAMS) {
        if constexpr (FIRST) row_wsum_lead<ANM_ROW_ARGS>(sr, si, wbb_r, wbp_r, wbb_i, wbp_i, wpb_r, nwpb_i, one);
        else row_wsum<ANM_ROW_ARGS>(sr, si, wpb_r, nwpb_i, one);
      });
    }
    const double fr = sr - bus_p, fi = si - bus_q;
    // row-wide stop test (see newton_groups)
    const unsigned long long badm = __builtin_amdgcn_fcmp(fmax(fabs(fr), fabs(fi)), tol, FCMP_UGT);
    const unsigned long long nanm = __builtin_amdgcn_fcmp(fr, fi, FCMP_UNO);
    tb = row_pick(badm, glo, ghi);
    tn = row_pick(nanm, glo, ghi);
    it = row_count(it, runm);   // the update applied in the previous trip
    runm &= __builtin_amdgcn_uicmp(tb, 0u, ICMP_NE) & ~__builtin_amdgcn_uicmp(tn, 0u, ICMP_NE) &
            __builtin_amdgcn_sicmp(it, max_iter, ICMP_SLT);   // NaN > tol is false, like the reference
    const bool all_done = runm == 0ull;   // (the loop is left at the END of the trip, see newton_groups)

    // ---- Jacobian blocks: own diagonal and the two couplings with the parent.  PAIRS: of Jpb MY ROW alone, (ja, jb),
    // selected once per trip: row 0 is (-nwpb_i, wpb_r), row 1 (-wpb_r, -nwpb_i)
    Blk<JT> Dg = Blk<JT>{JT(wbb_i - si), JT(sr + wbb_r), JT(sr - wbb_r), JT(si + wbb_i)};
    const Blk<JT> Jbp = Blk<JT>{JT(wbp_i), JT(wbp_r), JT(-wbp_r), JT(wbp_i)};
    [[maybe_unused]] Blk<JT> Jpb;
    [[maybe_unused]] JT ja, jb;
    if constexpr (PAIRS) {
      const JT jpr = JT(wpb_r), jpi = JT(nwpb_i);
      ja = -(rep ? jpr : jpi); jb = row_flip(rep ? jpi : jpr, flip);
    } else {
      Jpb = Blk<JT>{JT(-nwpb_i), JT(wpb_r), JT(-wpb_r), JT(-nwpb_i)};
    }
    JT r0 = JT(fr), r1 = JT(fi);
    // ---- The unconditional schedule.  EVERY lane runs every level's pivot code and every depth's step code; no level and
    // no depth is a region.  A bus still ends with the bits of "pivot at my height, step at my depth":
    //   * Dg, r0 and r1 of a bus are destinations of folds only at levels up to its own height, and r0 / r1 of a parent's
    //     step only at its own depth (a bus attached to the slack: never) -- tests/test_row_plan.py, test_row_schedule.py;
    //   * so what a lane computes BEFORE its level (depth) is overwritten before anybody reads it -- the hand-over of a bus
    //     of height h is read at level h + 1, its step at depth + 1 -- and what it computes AFTER repeats the same
    //     operations on unchanged operands.
    // Hence also one place for the step of the buses attached to the slack: d = Di r at the head of the back substitution,
    // after the last level, whatever their heights.
    // ---- elimination by height: the folds of a level (every child of height h - 1 into its parent, whatever the parent's
    // height), then the pivot.  Lr = Lk r is finished by the lead of the next level's folds (Lr0 / Lr1 hold Lk.b r1, Lk.d r1).
    // PAIRS: (Sc.a, Sc.b) is MY ROW of Sc, Lr0 my entry of Lr and Lka my Lk.a, resp. Lk.c; Sc.c, Sc.d, Lr1 and Lkc are not
    // used.  Sc.b is finished by the lead as well (it holds Lk.b Jbp.d, resp. Lk.d Jbp.d).
    Blk<JT> Di = Dg, Sc = Dg;
    JT Lr0 = JT(0), Lr1 = JT(0), Lka = JT(0), Lkc = JT(0);
    static_for<0, T::T_MAXH + 1>([&](auto H) {
      constexpr int h = H;
      if constexpr (h > 0) {
        static_assert(T::T_ROW_CH_OFF[h + 1] > T::T_ROW_CH_OFF[h], "a level above 0 folds the child that makes it one");
        row_points<T, PAIRS ? ROW_CH_PAIR : ROW_CH, T::T_ROW_CH_OFF[h], T::T_ROW_CH_OFF[h + 1]>([&](auto FIRST, ANM_ROW_PARAMS) {
          if constexpr (PAIRS) {
            if constexpr (FIRST) row_pair_fold_lead<ANM_ROW_ARGS>(Dg, r0, r1, Sc.a, Sc.b, Lr0, Lka, Jbp.b, onej);
            else row_pair_fold<ANM_ROW_ARGS>(Dg, r0, r1, Sc.a, Sc.b, Lr0, onej);
          } else {
            if constexpr (FIRST) row_fold_lead<ANM_ROW_ARGS>(Dg, r0, r1, Sc, Lr0, Lr1, Lka, Lkc, onej);
            else row_fold<ANM_ROW_ARGS>(Dg, r0, r1, Sc, Lr0, Lr1, onej);
          }
        });
      }
      Di = blk_inv_fast(Dg);
      if constexpr (h < T::T_MAXH) {
        if constexpr (PAIRS) {
          Lka = fm(ja, Di.a, jb * Di.c);                 // blk_mul(Jpb, Di), my row
          const JT Lkb = fm(ja, Di.b, jb * Di.d);
          Sc.a = fm(Lka, Jbp.a, Lkb * Jbp.c);            // blk_mul(Lk, Jbp), my row
          Sc.b = Lkb * Jbp.d;
          Lr0 = Lkb * r1;
        } else {
          const Blk<JT> Lk = blk_mul(Jpb, Di);
          Sc = blk_mul(Lk, Jbp);
          Lr0 = Lk.b * r1; Lka = Lk.a;
          Lr1 = Lk.d * r1; Lkc = Lk.c;
        }
      }
    });
    // ---- back substitution by depth (Di holds the inverted pivots).  The step d = Di r of every lane leads the hand-over of
    // the next depth, where the parents' steps go straight into the right-hand sides of their children: the banks of a
    // hand-over hold buses of one depth, and r0 / r1 are rebuilt every trip.
    JT d0, d1;
    static_for<1, T::T_MAXD + 1>([&](auto Dd) {
      constexpr int dd = Dd;
      static_assert(T::T_ROW_PAR_OFF[dd + 1] > T::T_ROW_PAR_OFF[dd], "a depth above 0 has a parent's step to receive");
      row_points<T, ROW_PAR, T::T_ROW_PAR_OFF[dd], T::T_ROW_PAR_OFF[dd + 1]>([&](auto FIRST, ANM_ROW_PARAMS) {
        if constexpr (FIRST) row_step_lead<ANM_ROW_ARGS>(r0, r1, d0, d1, Di, Jbp.a, Jbp.b);
        else row_fma<ANM_ROW_ARGS>(r0, r1, d0, d1, Jbp.a, Jbp.b);
      });
    });
    d0 = fm(Di.a, r0, Di.b * r1);
    d1 = fm(Di.c, r0, Di.d * r1);
    // ---- update of the running rows
    update_iterate(runm, d0, d1, vm, cs, sn);
    if (all_done) break;
  }
}

// continue_in_groups with four solves a pass, one per row: the same LDS slots, the same results in st.it / st.diff.
// PAIRS: the topology has a pair plan, and the pass runs on two lanes per bus (newton_rows<.., true>; only replica 0 of a
// bus writes its results back) unless one_lane (uniform) asks for one.  The hand-over around the loop is instantiated ONCE
// for both: a second instantiation costs the kernels that hold an environment per lane 20 and more registers.
template <class T, class JT, bool PAIRS = false>
__device__ __forceinline__ void continue_in_rows(cptr_t C, EnvWork<T>& w, PFState<T>& st, bool mine, double tol, int max_iter,
                                                 double* lds, bool one_lane = true) {
  typedef Slot<T> S;
  constexpr int NR = 4;
  static_assert(Shape<T>::NG >= NR, "the hand-over slots of the wavefront hold a solve per row");
  const int lane = threadIdx.x & 63;
  const int row = lane >> 4;
  const bool pairs = PAIRS && !one_lane;
  RowView<T> V;
  V.init(C, pairs);
  const int b = V.b;
  const unsigned long long todo = __ballot(mine);
  const int n_todo = __popcll(todo);
  const int rank = __popcll(todo & ((1ull << lane) - 1ull));
  for (int base = 0; base < n_todo; base += NR) {
    const bool send = mine && rank >= base && rank < base + NR;
    if (send) slot_send<T>(lds + (rank - base) * S::SIZE, w, st);
    ANM_WAVE_SYNC();
    const bool rvalid = base + row < n_todo;           // this row holds a solve
    const bool isbus = V.lane_bus && rvalid;
    double vm = 1.0, cs = 1.0, sn = 0.0, bus_p = 0.0, bus_q = 0.0;
    int it = 0;
    if (isbus) slot_load<T>(lds + row * S::SIZE, b, vm, cs, sn, bus_p, bus_q);
    if (rvalid) it = int(lds[row * S::SIZE + S::IT]);
    ANM_WAVE_SYNC();
    unsigned tb, tn;
    if constexpr (PAIRS) {
      if (pairs) newton_rows<T, JT, true>(V, rvalid, vm, cs, sn, bus_p, bus_q, it, tb, tn, tol, max_iter);
      else newton_rows<T, JT, false>(V, rvalid, vm, cs, sn, bus_p, bus_q, it, tb, tn, tol, max_iter);
    } else {
      newton_rows<T, JT, false>(V, rvalid, vm, cs, sn, bus_p, bus_q, it, tb, tn, tol, max_iter);
    }

    // ---- results back to the owner lanes (V.rep: never set on one lane per bus)
    if (isbus && !V.rep) slot_store<T>(lds + row * S::SIZE, b, vm, cs, sn, it, tb, tn);
    ANM_WAVE_SYNC();
    if (send) {
      slot_receive<T>(lds + (rank - base) * S::SIZE, w, st);
      st.active = false;
    }
    ANM_WAVE_SYNC();
  }
}

// The collective continuation of a wavefront's handed-over solves, and the ONE place that chooses between rows and groups.
// Every path gives the same bits, so the choice is what is fastest: a pass lasts as long as its longest solve, and a
// diverging one runs to max_iter.  Rows take four solves a pass, groups 64 / GRP (eight for the 6-bus feeder) at a longer
// trip; two passes that each hold a diverging solve double the chain.  rowc (anm_solver_opts.row_continuation):
//    0  n <= 4 solves: rows.  More: groups up to iteration ANM_MID_CAP_DEFAULT (every converging solve seen needs <= 9),
//       then the survivors on rows if at most 4 are left, else on groups to the cap;
//    1  always rows;   -1  never;
//    2  the policy of 0 with the rows on ONE lane per bus even where the topology has a pair plan.
// A row pass runs on two lanes per bus (newton_rows<.., true>: a shorter trip) where the topology has a pair plan (T_ROW2),
// else on one.  A topology without a row plan (T_ROW = 0) keeps groups.
template <class T, class JT, bool ROWS = true>
__device__ __forceinline__ void continue_collective(cptr_t C, EnvWork<T>& w, PFState<T>& st, bool mine, double tol, int max_iter,
                                                    int rowc, double* lds) {
  if constexpr (T::T_ROW == 0 || !ROWS) {
    continue_in_groups<T, JT>(C, w, st, mine, tol, max_iter, lds);
  } else {
    const bool policy = rowc == 0 || rowc == 2;
    int n = __popcll(__ballot(mine));
    bool groups = rowc < 0 || (policy && n > 4);
    int cap = (policy && ANM_MID_CAP_DEFAULT < max_iter) ? ANM_MID_CAP_DEFAULT : max_iter;
    while (groups) {
      continue_in_groups<T, JT>(C, w, st, mine, tol, cap, lds, cap < max_iter);
      mine = mine && st.active;   // (at the cap: nobody)
      n = __popcll(__ballot(mine));
      groups = n > 4;
      cap = max_iter;
    }
    if (n > 0) continue_in_rows<T, JT, T::T_ROW2 != 0>(C, w, st, mine, tol, max_iter, lds, rowc == 2);
  }
}

}  // namespace group
}  // namespace anm
#endif  // __HIPCC__
