// rtc_model.hpp -- the Model adapter of a run-time compiled device model (c3sc_hip_model_compile, rtc.hip).
//
// rtc.hip compiles one program per model with hipRTC: this header, the kernel headers it includes, and before them the
// user's source wrapped in namespace c3sc_user, which defines (include/c3sc_hip.h states the contract)
//   drift(prm, x, u, b)  sigma(prm, x, u, s)  stage(prm, x, u)  boundcost(prm, x)  obscost(prm, x)
// and, for a stopping model, stopcost(prm, x); for a jump-diffusion model, jumprate(prm, x) and
// jump(prm, x, m, y); for an impulse-control model, impulse(prm, x, m, y); for a model with correlated noise
// (DESIGN.md 4.16), covar(prm, x, p)
// with C3SC_D / C3SC_DU defined.  RtcModel presents them as the Model concept of models.hpp: no tables and no candidate
// features (the user's code evaluates its own transcendentals with the device libm), an empty Node.  The masks come from the
// spec; their safe defaults (every dimension depends on u, none is a constant of the candidate, the stage cost reads u) are
// resolved by rtc.hip.  The optional traits (STAGE_USEP, HAS_DEPS, CF_FROM_U) are not defined: the kernels then take their
// general paths.
#pragma once
#include "kernel_fiber_per_wave.hpp"
#include "kernel_rollout_ode.hpp"
#include "models.hpp"

namespace c3sc {

template <int DIM, int NU, unsigned UDEP, unsigned UCONST, bool SUDEP>
struct RtcModel {
    static constexpr bool IS_TABLE = false;
    static constexpr int D = DIM, DU = NU;
    static constexpr int NTAB = 0, NCF = 0;
    static constexpr unsigned UDEP_MASK = UDEP, UCONST_MASK = UCONST;
    static constexpr bool STAGE_UDEP = SUDEP;
    __host__ __device__ static constexpr int tab_dim(int) { return 0; }
    struct Node {};
    __device__ static inline void prep(const double *, const double (&)[D], const double (&)[1], Node &) {}
    __device__ static inline void drift(const double *prm, const Node &, const double (&x)[D], const double *u, const double *,
                                        double (&b)[D])
    {
        ::c3sc_user::drift(prm, x, u, b);
    }
    __device__ static inline void sigma(const double *prm, const double (&x)[D], const double *u, double (&s)[D])
    {
        ::c3sc_user::sigma(prm, x, u, s);
    }
    __device__ static inline double stage(const double *prm, const double (&x)[D], const double *u)
    {
        return ::c3sc_user::stage(prm, x, u);
    }
    __device__ static inline double boundcost(const double *prm, const double (&x)[D]) { return ::c3sc_user::boundcost(prm, x); }
    __device__ static inline double obscost(const double *prm, const double (&x)[D]) { return ::c3sc_user::obscost(prm, x); }
#ifdef C3SC_RTC_STOP // a spec with the stop flag (c3sc_hip_model_compile_os): only then must the source define stopcost
    __device__ static inline double stopcost(const double *prm, const double (&x)[D]) { return ::c3sc_user::stopcost(prm, x); }
#endif
#ifdef C3SC_RTC_JUMP // a spec with njump > 0 (c3sc_hip_model_compile_jd): only then must the source define jumprate and jump
    static constexpr int NJUMP = C3SC_NJUMP;
    __device__ static inline double jumprate(const double *prm, const double (&x)[D]) { return ::c3sc_user::jumprate(prm, x); }
    __device__ static inline double jump(const double *prm, const double (&x)[D], int m, double (&y)[D])
    {
        return ::c3sc_user::jump(prm, x, m, y);
    }
#endif
#ifdef C3SC_RTC_IMPULSE // a spec with nimpulse > 0 (c3sc_hip_model_compile_ic): only then must the source define impulse
    static constexpr int NIMPULSE = C3SC_NIMPULSE;
    __device__ static inline double impulse(const double *prm, const double (&x)[D], int m, double (&y)[D])
    {
        return ::c3sc_user::impulse(prm, x, m, y);
    }
#endif
#ifdef C3SC_RTC_CORR // a spec with ncorr > 0 (c3sc_hip_model_compile_cd): only then must the source define covar
    static constexpr int NCORR = C3SC_NCORR;
    static constexpr int CORR_I[C3SC_NCORR] = {C3SC_CORR_I}, CORR_J[C3SC_NCORR] = {C3SC_CORR_J};
    __device__ static inline double covar(const double *prm, const double (&x)[D], int p) { return ::c3sc_user::covar(prm, x, p); }
#endif
};

} // namespace c3sc
