// dotnet_minmax.hpp -- .NET Framework's Math.Max / Math.Min on doubles, shared by
// sens_ranging_kernels.hip (lpr_sens_ranging)
// and sens_batch_ranging_kernels.hip (lpr_sens_batch_ranging, section 19).  Device code only.
#pragma once

#include "engine_common.hpp"

namespace lpr {

// .NET Framework Math.Max / Math.Min on doubles (oracle/oracle_revised.c:90 quotes Max)
__device__ __forceinline__ double dn_max(double a, double b) {
    if (a > b) return a;
    if (a != a) return a;
    return b;
}
__device__ __forceinline__ double dn_min(double a, double b) {
    if (a < b) return a;
    if (a != a) return a;
    return b;
}

}  // namespace lpr
