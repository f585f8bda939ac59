// hsim device renderer: the host launcher of the ray-cast kernel (hs_render.hip) behind
// hs_render_frames.  Replaces mujoco.Renderer.render() on the reference's video path
// (custom_env.py:273-289) for many frames at once; render.py's host ray caster is the same
// arithmetic and serves as its oracle.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hs_model.h"

namespace hs {

enum { CAM_BODY = 0, CAM_COM = 1 };   // include/hsim.h HS_CAM_BODY / HS_CAM_COM

// what the kernel needs of the model (fp64, the host model's own values) and of the camera
struct RenderScene {
  int ngeom;
  int geom_type[MAXGEOM];
  double geom_r[MAXGEOM], geom_hl[MAXGEOM];   // geom_size[g][0], geom_size[g][1]
};
struct RenderCam {
  int mode, body;
  double pos[3], rot[9];   // rot row-major, columns x, y, z (the camera looks along -z)
  double f;                // focal length in pixels: 0.5 H / tan(fovy / 2)
};

// n frames from n kinematics records kin[n][KINDIM] (T = float or double) -> rgb[n][H][W][3]
template <typename T>
hipError_t launch_render(const T* kin, int n, const RenderScene& scene, const RenderCam& cam, int H, int W,
                         uint8_t* rgb, hipStream_t stream);

}  // namespace hs
