// The surface normal of a pixel from its neighbours in the ray image, shared by the ICP maps (tsdf_render.hip) and the shaded
// live view (tsdf_image.hip).  Files including this header are compiled with -ffp-contract=off.
#pragma once
#include "tsdf_common.hpp"

namespace gpst {

// computeNormalAndAngle<useSmoothing = true, flipNormals = false> (ITMVisualisationEngine_Shared.h:257-338) for a pixel whose own
// ray found the surface: the +-2 neighbours; the +-1 neighbours where one of those is missing or further away than 0.15 m.
// -> found; the unit normal and its angle against the light (-column 2 of invM) are valid when true.
__device__ __forceinline__ bool image_normal_and_angle(const float4* __restrict__ pr, int x, int y, int W, int H, float voxel_size,
                                                       const Mat4& invM, float& nx, float& ny, float& nz, float& angle) {
    if (y <= 2 || y >= H - 3 || x <= 2 || x >= W - 3) return false;
    float4 xp = pr[(x + 2) + y * W], yp = pr[x + (y + 2) * W], xm = pr[(x - 2) + y * W], ym = pr[x + (y - 2) * W];
    float dxx = 0.f, dxy = 0.f, dxz = 0.f, dyx = 0.f, dyy = 0.f, dyz = 0.f;
    bool doPlus1 = false;
    if (xp.w <= 0 || yp.w <= 0 || xm.w <= 0 || ym.w <= 0) doPlus1 = true;
    else {
        dxx = xp.x - xm.x; dxy = xp.y - xm.y; dxz = xp.z - xm.z;
        dyx = yp.x - ym.x; dyy = yp.y - ym.y; dyz = yp.z - ym.z;
        const float la = dxx * dxx + dxy * dxy + dxz * dxz, lb = dyx * dyx + dyy * dyy + dyz * dyz;
        const float ld = (la < lb) ? lb : la;
        if (ld * voxel_size * voxel_size > (0.15f * 0.15f)) doPlus1 = true;
    }
    if (doPlus1) {
        xp = pr[(x + 1) + y * W]; yp = pr[x + (y + 1) * W]; xm = pr[(x - 1) + y * W]; ym = pr[x + (y - 1) * W];
        dxx = xp.x - xm.x; dxy = xp.y - xm.y; dxz = xp.z - xm.z;
        dyx = yp.x - ym.x; dyy = yp.y - ym.y; dyz = yp.z - ym.z;
        if (xp.w <= 0 || yp.w <= 0 || xm.w <= 0 || ym.w <= 0) return false;
    }
    nx = -(dxy * dyz - dxz * dyy);
    ny = -(dxz * dyx - dxx * dyz);
    nz = -(dxx * dyy - dxy * dyx);
    const float ns = 1.0f / sqrtf(nx * nx + ny * ny + nz * nz);
    nx *= ns; ny *= ns; nz *= ns;
    angle = nx * (-invM.m[8]) + ny * (-invM.m[9]) + nz * (-invM.m[10]);
    return angle > 0.0;
}

}  // namespace gpst
