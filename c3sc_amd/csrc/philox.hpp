// philox.hpp -- counter-based normal noise of the batched closed-loop rollouts (c3sc_hip_simulate), shared by the device
// kernel and its host twin c3sc_hip_normals.
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) maps a 128-bit counter
// and a 64-bit key to 128 random bits.  key = the seed; counter = (trajectory index lo, hi, step, component pair).  One call
// gives two 53-bit uniforms and, by Box-Muller, the normals of components 2p and 2p+1: a trajectory's noise is a function
// of (seed, global trajectory index, step, component) alone -- not of the batch size, the launch split or the thread mapping.
//
// Box-Muller needs log, cos and sin.  They are written out here (range reduction by exact bit / octant arithmetic, fixed
// polynomials, every multiply-add an explicit fma, contraction off) so that host and device produce the SAME bits and the
// noise costs no data-dependent branch.  Accuracy: a few ulp, far below what a noise sample needs.
#pragma once
#ifdef __HIPCC_RTC__
#include "rtc_prelude.hpp"
#else
#include <hip/hip_runtime.h>

#include <stdint.h>
#endif

namespace c3sc {

struct Philox4 {
    uint32_t v[4];
};

__host__ __device__ inline void philox_mulhilo(uint32_t a, uint32_t b, uint32_t &hi, uint32_t &lo)
{
    const uint64_t p = (uint64_t)a * (uint64_t)b;
    hi = (uint32_t)(p >> 32);
    lo = (uint32_t)p;
}

// Philox4x32 with 10 rounds (Random123's philox4x32_R(10, ...)): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key bumps
// 0x9E3779B9 / 0xBB67AE85 between rounds
__host__ __device__ inline Philox4 philox4x32_10(Philox4 c, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        uint32_t hi0, lo0, hi1, lo1;
        philox_mulhilo(0xD2511F53u, c.v[0], hi0, lo0);
        philox_mulhilo(0xCD9E8D57u, c.v[2], hi1, lo1);
        const Philox4 n = {{hi1 ^ c.v[1] ^ k0, lo1, hi0 ^ c.v[3] ^ k1, lo0}};
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// (0, 1): the top 53 bits of a 64-bit word, centred in their interval (never 0, never 1)
__host__ __device__ inline double u53(uint32_t hi, uint32_t lo)
{
    const uint64_t w = ((uint64_t)hi << 32) | lo;
    return ((double)(w >> 11) + 0.5) * 0x1.0p-53;
}

// log(u) for u in (0, 1): u = 2^e m with m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s), s = (m - 1) / (m + 1), |s| <= 0.1716;
// the odd series to s^23 (next term < 2^-60 relative)
__host__ __device__ inline double bm_log(double u)
{
#pragma clang fp contract(off)
    uint64_t b;
    __builtin_memcpy(&b, &u, 8);
    int e = (int)((b >> 52) & 0x7ff) - 1023;
    uint64_t mb = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull; // m in [1, 2)
    double m;
    __builtin_memcpy(&m, &mb, 8);
    const bool big = m >= 1.4142135623730951;
    m = big ? m * 0.5 : m; // exact
    e = big ? e + 1 : e;
    const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
    double p = 1.0 / 23.0;
    p = fma(p, s2, 1.0 / 21.0);
    p = fma(p, s2, 1.0 / 19.0);
    p = fma(p, s2, 1.0 / 17.0);
    p = fma(p, s2, 1.0 / 15.0);
    p = fma(p, s2, 1.0 / 13.0);
    p = fma(p, s2, 1.0 / 11.0);
    p = fma(p, s2, 1.0 / 9.0);
    p = fma(p, s2, 1.0 / 7.0);
    p = fma(p, s2, 1.0 / 5.0);
    p = fma(p, s2, 1.0 / 3.0);
    const double lm = 2.0 * fma(s * s2, p, s);
    return fma((double)e, 0.69314718055994531, lm);
}

// cos(2 pi u), sin(2 pi u) for u in [0, 1): the octant is taken from u exactly (u = (q + f) / 8, |f| <= 1/2), the
// remainder r = f pi / 4 lies in [-pi/8, pi/8]; Taylor polynomials to r^20 / r^21 (truncation < 2^-70)
__host__ __device__ inline void bm_sincos2pi(double u, double &sn, double &cs)
{
#pragma clang fp contract(off)
    const double t = u * 8.0; // exact
    const double q = rint(t), f = t - q; // exact
    const int oct = ((int)q) & 7;
    const double r = f * 0.78539816339744831, r2 = r * r;
    double ps = -1.0 / 51090942171709440000.0; // -1/21!
    ps = fma(ps, r2, 1.0 / 121645100408832000.0);
    ps = fma(ps, r2, -1.0 / 355687428096000.0);
    ps = fma(ps, r2, 1.0 / 1307674368000.0);
    ps = fma(ps, r2, -1.0 / 6227020800.0);
    ps = fma(ps, r2, 1.0 / 39916800.0);
    ps = fma(ps, r2, -1.0 / 362880.0);
    ps = fma(ps, r2, 1.0 / 5040.0);
    ps = fma(ps, r2, -1.0 / 120.0);
    ps = fma(ps, r2, 1.0 / 6.0);
    const double sr = fma(-r * r2, ps, r);
    double pc = 1.0 / 2432902008176640000.0; // 1/20!
    pc = fma(pc, r2, -1.0 / 6402373705728000.0);
    pc = fma(pc, r2, 1.0 / 20922789888000.0);
    pc = fma(pc, r2, -1.0 / 87178291200.0);
    pc = fma(pc, r2, 1.0 / 479001600.0);
    pc = fma(pc, r2, -1.0 / 3628800.0);
    pc = fma(pc, r2, 1.0 / 40320.0);
    pc = fma(pc, r2, -1.0 / 720.0);
    pc = fma(pc, r2, 1.0 / 24.0);
    pc = fma(pc, r2, -1.0 / 2.0);
    const double cr = fma(r2, pc, 1.0);
    // angle = oct * pi/4 + r; with c = cos(pi/4) = sin(pi/4), odd octants mix the two
    const double c4 = 0.70710678118654752;
    const double cm = c4 * (cr - sr), cp = c4 * (cr + sr); // cos(pi/4 + r), sin(pi/4 + r)
    double C = cr, S = sr;
    C = (oct == 1) ? cm : C;  S = (oct == 1) ? cp : S;
    C = (oct == 2) ? -sr : C; S = (oct == 2) ? cr : S;
    C = (oct == 3) ? -cp : C; S = (oct == 3) ? cm : S;
    C = (oct == 4) ? -cr : C; S = (oct == 4) ? -sr : S;
    C = (oct == 5) ? -cm : C; S = (oct == 5) ? -cp : S;
    C = (oct == 6) ? sr : C;  S = (oct == 6) ? -cr : S;
    C = (oct == 7) ? cp : C;  S = (oct == 7) ? -cm : S;
    sn = S;
    cs = C;
}

// the standard normal of component j (0-based) of step `step` of global trajectory `traj` under key `seed`
__host__ __device__ inline double philox_normal(uint64_t seed, uint64_t traj, uint32_t step, uint32_t j)
{
#pragma clang fp contract(off)
    const Philox4 c = {{(uint32_t)traj, (uint32_t)(traj >> 32), step, j >> 1}};
    const Philox4 o = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u1 = u53(o.v[0], o.v[1]), u2 = u53(o.v[2], o.v[3]);
    const double rr = sqrt(-2.0 * bm_log(u1));
    double sn, cs;
    bm_sincos2pi(u2, sn, cs);
    return rr * ((j & 1u) ? sn : cs);
}

// the two uniforms of the compound-Poisson increment of step `step` of global trajectory `traj`: the event
// test and the mark.  Counter component 0x80000000: the normals use j >> 1 there, far below it, so no normal shares a counter
// with them and the diffusion noise of a run keeps its bits whether or not the model jumps
__host__ __device__ inline void philox_jump_uniforms(uint64_t seed, uint64_t traj, uint32_t step, double &u0, double &u1)
{
    const Philox4 c = {{(uint32_t)traj, (uint32_t)(traj >> 32), step, 0x80000000u}};
    const Philox4 o = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    u0 = u53(o.v[0], o.v[1]);
    u1 = u53(o.v[2], o.v[3]);
}

} // namespace c3sc
