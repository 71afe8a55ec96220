// The counter-based sampler of the sampling solvers: gmpc_cem.hip, gmpc_mppi.hip and
// gmpc_icem.hip (through gmpc_cem_rollout.h) include it.  A control is a pure function of (seed, iteration, problem, sample, step, control) -- cem_control, the one place
// a control is formed -- so no kernel stores noise or samples: each regenerates what it needs.  (CemRng itself is in
// gmpc_launch.h, beside the argument blocks that carry it.)
#pragma once
#include "gmpc_launch.h"

// ---- the sampler ----------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al. 2011): counter c, key k -> four words
__device__ __forceinline__ void cem_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                           uint32_t k1, uint32_t (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// z[s][e] of problem b, e = t m + j: word e & 3 of the group e >> 2.  u = ((r >> 9) 2 + 1) 2^-24 is exact and inside
// (0, 1); the angle 2 pi u is taken by sinpi / cospi of the exact 2 u, so no rounding of the angle reaches z.
__device__ __forceinline__ float cem_normal(const CemRng& g, int b, int s, int e) {
  uint32_t r[4];
  cem_philox((uint32_t)(e >> 2), (uint32_t)s, (uint32_t)b, g.it, g.key0, g.key1, r);
  const uint32_t ra = (e & 2) ? r[2] : r[0], rb = (e & 2) ? r[3] : r[1];
  const float ua = (float)((ra >> 9) * 2u + 1u) * 0x1p-24f, ub = (float)((rb >> 9) * 2u + 1u) * 0x1p-24f;
  const float rad = sqrtf(-2.f * logf(ua));
  return rad * ((e & 1) ? sinpif(2.f * ub) : cospif(2.f * ub));
}

// The control j of step t of sample s of problem b: the only place a control is formed (k_cem_rollout and k_cem_update
// both call it).  Smoothing along time zt_0 = z_0, zt_t = beta zt_{t-1} + cbeta z_t, run from step 0 (beta = 0: z_t
// itself, the same value); the clamp is two selects, so a NaN stays a NaN.  lo / hi: -inf / +inf when unbounded.
__device__ __forceinline__ float cem_control(const CemRng& g, int b, int s, int t, int j, int m, float mean, float sd,
                                             float lo, float hi) {
  float z;
  if (g.beta == 0.f) {
    z = cem_normal(g, b, s, t * m + j);
  } else {
    z = cem_normal(g, b, s, j);
    for (int tt = 1; tt <= t; ++tt)
      z = __fadd_rn(__fmul_rn(g.beta, z), __fmul_rn(g.cbeta, cem_normal(g, b, s, tt * m + j)));
  }
  float u = fmaf(sd, z, mean);
  u = u < lo ? lo : u;
  u = u > hi ? hi : u;
  return u;
}
