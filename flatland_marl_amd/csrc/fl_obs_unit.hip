// fl_obs_unit.hip -- the source of EVERY observation-kernel translation unit.  build.sh compiles it once per unit of its list, each time
// with the defines that say which instantiation of fl_obs_body.h the unit holds (one kernel body per object: the units compile in
// parallel and their code generation does not depend on each other -- the kernel sits at its 128-VGPR ceiling):
//   -DFL_OBS_UNIT_MODE=k                           (unit mk)   the runtime-carving kernels of MODE k: k_obs<k, VAR> for VAR 0 / 1 / 2
//   -DFL_OBS_UNIT_CLASS=K                          (unit fK)   launch class K: k_obs<MODE, VAR, K>, MODE and VAR the class's
//   -DFL_OBS_UNIT_CLASS=K -DFL_OBS_UNIT_CLASS2=K2  (unit sK*)  the split kernel k_obs_split<MODE, VAR, K, K2>: class K's body for the envs
//                                                              that fit it, class K2's (0: the runtime carving's) for the others
// The launchers are the templates fl_obs_launch_mode / fl_obs_launch_class that fl_obs_layout.h declares and fl_obs.hip calls: a kernel
// that fl_obs.hip names and no unit of the build instantiates is an undefined symbol of the library.
#include "fl_obs_body.h"

template <typename KernelT>
static int obs_launch(KernelT kern, const FlDev &d, const FlObsScratch &o, const ObsArgs &P, hipStream_t s) {
    if (hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return FL_ERR_HIP;
    hipLaunchKernelGGL(kern, dim3(d.B), dim3(P.L.nt), P.L.total, s, d, o, P);
    return FL_OK;
}

template <int MODE>
int fl_obs_launch_mode(int var, const FlDev &d, const FlObsScratch &o, const ObsArgs &P, hipStream_t s) {
    if constexpr (MODE == 5) {
        if (var == 1) return FL_ERR_ARG;   // (both builders in rounds of 16 agents: the static tables never join a launch this tight on LDS)
    } else {
        if (var == 1) return obs_launch(k_obs<MODE, 1>, d, o, P, s);
    }
    return var == 2 ? obs_launch(k_obs<MODE, 2>, d, o, P, s) : obs_launch(k_obs<MODE, 0>, d, o, P, s);
}

template <int FIX, int FIX2>
int fl_obs_launch_class(const FlDev &d, const FlObsScratch &o, const ObsArgs &P, hipStream_t s) {
    using F = ObsFixed<FIX>;
    constexpr int MODE = obs_fixed_mode<FIX>(), VAR = obs_fixed_var<FIX>();
    static_assert(F::L.total <= 160 * 1024 || F::opt.nh, "the class's carving fits the LDS of a CU");
    static_assert(F::shape.merged != 3 || F::L.total <= 80 * 1024, "rounds of 16 agents on 512 threads: two workgroups a CU");
    if constexpr (FIX2 < 0) return obs_launch(k_obs<MODE, VAR, FIX>, d, o, P, s);
    else {
        static_assert(FIX2 == 0 || (obs_fixed_mode<FIX2 != 0 ? FIX2 : FIX>() == MODE && obs_fixed_var<FIX2 != 0 ? FIX2 : FIX>() == VAR),
                      "both bodies of a split kernel are the same MODE and VAR");
        return obs_launch(k_obs_split<MODE, VAR, FIX, FIX2>, d, o, P, s);
    }
}

#if defined(FL_OBS_UNIT_MODE) && !defined(FL_OBS_UNIT_CLASS)
template int fl_obs_launch_mode<FL_OBS_UNIT_MODE>(int, const FlDev &, const FlObsScratch &, const ObsArgs &, hipStream_t);
#elif defined(FL_OBS_UNIT_CLASS) && !defined(FL_OBS_UNIT_MODE)
#ifndef FL_OBS_UNIT_CLASS2
#define FL_OBS_UNIT_CLASS2 -1   // not a split kernel
#endif
template int fl_obs_launch_class<FL_OBS_UNIT_CLASS, FL_OBS_UNIT_CLASS2>(const FlDev &, const FlObsScratch &, const ObsArgs &, hipStream_t);
#else
#error "fl_obs_unit.hip: define FL_OBS_UNIT_MODE or FL_OBS_UNIT_CLASS (build.sh: obs_unit_defines)"
#endif
