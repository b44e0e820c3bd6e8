// The Vina scoring function on the device, stated once: the XS type table, the term weights and the five pair terms
// (diffbindfr_amd/vina.py and docs/vina.md hold the full statement).  k_vina and k_vina_search (vina.hip) take the terms with
// their derivative, k_vina_decompose (decompose.hip) without; both files are built with the same floating-point flags
// (build.py), so a pair has the same five fp32 values in all of them.
#pragma once

#define V_DUMMY 16
#define V_NTYPES 18                   // XS types 0..15 and Met_D (17); 16 and anything outside 0..17 is DUMMY
#define V_CUTOFF 8.0f

// XS type table: radius, hydrophobic, donor, acceptor (row 16, DUMMY, is never read: v_typed).  The tables keep external linkage:
// with internal linkage the compiler folds their contents into the kernels, and the register allocation of k_vina and
// k_vina_decompose, which is pinned, moves.  Two __constant__ tables of one library cannot share a name, so every .hip names its
// copy before it includes this header.
#if !defined(VINA_XS_RAD) || !defined(VINA_XS_FLAGS)
#error "define VINA_XS_RAD and VINA_XS_FLAGS, this translation unit's names of the XS table, before including vina_terms.h"
#endif
//                                       C_H  C_P  N_P  N_D  N_A  N_DA O_P  O_D  O_A  O_DA S_P  P_P  F_H  Cl_H Br_H I_H  DUMMY Met_D
__constant__ float VINA_XS_RAD[V_NTYPES] = {1.9f, 1.9f, 1.8f, 1.8f, 1.8f, 1.8f, 1.7f, 1.7f, 1.7f, 1.7f, 2.0f, 2.1f, 1.5f, 1.8f, 2.0f, 2.2f, 0.f, 1.2f};
__constant__ int VINA_XS_FLAGS[V_NTYPES] = {1, 0, 0, 2, 4, 6, 0, 2, 4, 6, 0, 0, 1, 1, 1, 1, 0, 2};   // 1 hydrophobic, 2 donor, 4 acceptor

__device__ __forceinline__ bool v_typed(int t) { return t >= 0 && t < V_NTYPES && t != V_DUMMY; }

#define W_GAUSS1 (-0.035579f)
#define W_GAUSS2 (-0.005156f)
#define W_REPULSION 0.840245f
#define W_HYDROPHOBIC (-0.035069f)
#define W_HBOND (-0.587439f)
#define W_NROT 0.05846f

// One pair: the five weighted inter terms into t5[0..4]; with DERIV the return value is dE/dd of their sum (else 0).
template <bool DERIV> __device__ __forceinline__ float pair_terms(int ti, int tj, float r, float* t5) {
  const float d = r - VINA_XS_RAD[ti] - VINA_XS_RAD[tj];
  const int fi = VINA_XS_FLAGS[ti], fj = VINA_XS_FLAGS[tj];
  const float q1 = d * 2.f;                              // d / 0.5
  const float g1 = expf(-q1 * q1);
  const float q2 = (d - 3.f) * 0.5f;
  const float g2 = expf(-q2 * q2);
  float de = 0.f;
  if constexpr (DERIV) de = W_GAUSS1 * g1 * (-2.f * q1 * 2.f) + W_GAUSS2 * g2 * (-2.f * q2 * 0.5f);
  t5[0] = W_GAUSS1 * g1;
  t5[1] = W_GAUSS2 * g2;
  t5[2] = 0.f; t5[3] = 0.f; t5[4] = 0.f;
  if (d < 0.f) {
    t5[2] = W_REPULSION * (d * d);
    if constexpr (DERIV) de += W_REPULSION * 2.f * d;
  }
  if ((fi & 1) && (fj & 1)) {
    if (d < 0.5f) t5[3] = W_HYDROPHOBIC;
    else if (d < 1.5f) {
      t5[3] = W_HYDROPHOBIC * (1.5f - d);
      if constexpr (DERIV) de -= W_HYDROPHOBIC;
    }
  }
  if (((fi & 2) && (fj & 4)) || ((fi & 4) && (fj & 2))) {
    if (d < -0.7f) t5[4] = W_HBOND;
    else if (d < 0.f) {
      t5[4] = W_HBOND * (-d / 0.7f);
      if constexpr (DERIV) de -= W_HBOND / 0.7f;
    }
  }
  return de;
}
