// Real spherical-harmonics basis constants (upstream's SH_C0..SH_C3), shared by
// the preprocess colour evaluation (raster_pre.hip) and the per-Gaussian
// backward (raster_bwd.hip).  Each translation unit gets its own copy of the
// __constant__ arrays (internal linkage).
#pragma once

#include <hip/hip_runtime.h>

namespace wgsr {

namespace {

constexpr float SH_C0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.4886025119029199f;
__constant__ float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                               -1.0925484305920792f, 0.5462742152960396f};
__constant__ float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                               0.3731763325901154f,  -0.4570457994644658f, 1.445305721320277f,
                               -0.5900435899266435f};

}  // namespace

}  // namespace wgsr
