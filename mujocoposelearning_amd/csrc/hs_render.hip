// hsim device renderer for gfx950 (MI355X): the ray-cast kernel behind hs_render_frames.
//
// Replaces mujoco.Renderer.update_scene + render (custom_env.py:273-289) for n frames in one launch:
// n kinematics records (kin_batch_kernel's layout, hs_kernels.h KINDIM) in, uint8 rgb[n][H][W][3] out.
// The arithmetic is render.py's (Renderer.render / _capsule_hit / _sphere_hit / _shade), in fp64 and
// in the same operation order with contraction off, so the host renderer is this kernel's oracle;
// what depends on the frame only (camera pose, capsule end points, the ray-independent terms of the
// intersection tests) is computed once per workgroup into LDS, by the same expressions.
//
// Mapping: one thread per pixel, one workgroup of 256 threads per 16 x 16 pixel tile (a wave covers
// 4 rows of 16 pixels), the frame index in gridDim.z.  Every geom is tested for every pixel (the
// host's screen-space footprint is a conservative cull, so the image is the same); the scene reads
// are same-address LDS broadcasts.
#include "hs_render.h"

#include <algorithm>

#include "hs_kernels.h"

#pragma clang fp contract(off)

namespace hs {
namespace {

constexpr int TILE = 16;
constexpr double INF = __builtin_huge_val();

// humanoid.xml:28-31: the "body" material, the checker "grid" texture, the gradient skybox
__device__ constexpr double BODY_RGB[3] = {0.8, 0.6, 0.4};
__device__ constexpr double FLOOR_RGB[2][3] = {{0.1, 0.2, 0.3}, {0.2, 0.3, 0.4}};
__device__ constexpr double SKY_TOP[3] = {0.3, 0.5, 0.7};

struct SceneGeom {
  int type;
  double a[3], ax[3];             // capsule end gpos - hl ax (sphere: the centre; plane: its point), z-axis
  double oa[3], ob[3], ba[3];     // cpos - a, cpos - b, b - a
  double baba, baoa, k0;          // _capsule_hit's ray-independent terms
  double cca, ccb;                // oa.oa - r r, ob.ob - r r (the caps; cca is also _sphere_hit's cc)
  double hl2;                     // 2 hl (shading: the clamp of the axis coordinate)
  double num;                     // plane: (gpos - cpos) . normal
};

struct Scene {
  double cpos[3], R[9], light[3];
  int ngeom;
  SceneGeom g[MAXGEOM];
};

__device__ __forceinline__ double dot3(const double* a, const double* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
__device__ __forceinline__ double clip01(double x) { return fmin(fmax(x, 0.0), 1.0); }

template <typename T>
__global__ __launch_bounds__(TILE* TILE) void render_kernel(const T* __restrict__ kin, RenderScene sc, RenderCam cam,
                                                           int H, int W, uint8_t* __restrict__ rgb) {
  __shared__ Scene s;
  const int tid = threadIdx.x;
  const size_t frame = blockIdx.z;
  const T* rec = kin + frame * KINDIM;
  const T* xpos = rec;
  const T* xmat = rec + MAXBODY * 3;
  const T* gpos = rec + MAXBODY * 12;
  const T* gax = gpos + MAXGEOM * 3;
  const T* com = gax + MAXGEOM * 3;

  // -- the frame's camera and light (Renderer._camera_pose) --------------------------------------
  if (tid < 3) {
    const int i = tid;
    if (cam.mode == CAM_BODY) {
      const T* bR = xmat + cam.body * 9 + i * 3;
      const double r0 = (double)bR[0], r1 = (double)bR[1], r2 = (double)bR[2];
      s.cpos[i] = (double)xpos[cam.body * 3 + i] + (r0 * cam.pos[0] + r1 * cam.pos[1] + r2 * cam.pos[2]);
      for (int j = 0; j < 3; j++) s.R[i * 3 + j] = r0 * cam.rot[j] + r1 * cam.rot[3 + j] + r2 * cam.rot[6 + j];
    } else {
      s.cpos[i] = (double)com[i] + cam.pos[i];
      for (int j = 0; j < 3; j++) s.R[i * 3 + j] = cam.rot[i * 3 + j];
    }
    s.light[i] = (double)com[i] + (i == 2 ? 2.0 : 0.0);   // humanoid.xml:107 "top", trackcom
    if (i == 0) s.ngeom = sc.ngeom;
  }
  __syncthreads();
  // -- the frame's geoms ---------------------------------------------------------------------------
  if (tid < sc.ngeom) {
    SceneGeom& g = s.g[tid];
    const int typ = sc.geom_type[tid];
    const double r = sc.geom_r[tid], hl = typ == GEOM_CAPSULE ? sc.geom_hl[tid] : 0.0;
    g.type = typ;
    g.hl2 = 2 * hl;
    double b[3], gp[3];
    for (int k = 0; k < 3; k++) {
      gp[k] = (double)gpos[tid * 3 + k];
      g.ax[k] = (double)gax[tid * 3 + k];
    }
    if (typ == GEOM_PLANE) {
      double rel[3];
      for (int k = 0; k < 3; k++) {
        g.a[k] = gp[k];
        rel[k] = gp[k] - s.cpos[k];
      }
      g.num = dot3(rel, g.ax);
    } else {
      for (int k = 0; k < 3; k++) {
        g.a[k] = typ == GEOM_CAPSULE ? gp[k] - hl * g.ax[k] : gp[k];
        b[k] = typ == GEOM_CAPSULE ? gp[k] + hl * g.ax[k] : gp[k];
        g.ba[k] = b[k] - g.a[k];
        g.oa[k] = s.cpos[k] - g.a[k];
        g.ob[k] = s.cpos[k] - b[k];
      }
      g.baba = dot3(g.ba, g.ba);
      g.baoa = dot3(g.oa, g.ba);
      const double oaoa = dot3(g.oa, g.oa);
      g.k0 = g.baba * oaoa - g.baoa * g.baoa - r * r * g.baba;
      g.cca = oaoa - r * r;
      g.ccb = dot3(g.ob, g.ob) - r * r;
      g.num = 0;
    }
  }
  __syncthreads();

  // -- the pixel's ray (Renderer.render) ------------------------------------------------------------
  const int x = blockIdx.x * TILE + (tid & (TILE - 1)), y = blockIdx.y * TILE + tid / TILE;
  const double u = (x + 0.5 - 0.5 * W) / cam.f, v = (0.5 * H - y - 0.5) / cam.f;
  double d[3];
  for (int k = 0; k < 3; k++) d[k] = u * s.R[k * 3] + v * s.R[k * 3 + 1] - s.R[k * 3 + 2];
  const double dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  for (int k = 0; k < 3; k++) d[k] = d[k] / dn;

  // -- the nearest hit, geoms in index order (strict <: the lowest index wins a tie) ---------------
  double tbest = INF;
  int gid = -1;
  const int ng = s.ngeom;
  for (int gi = 0; gi < ng; gi++) {
    const SceneGeom& g = s.g[gi];
    double t = INF;
    if (g.type == GEOM_PLANE) {
      const double den = dot3(d, g.ax);
      const double tp = g.num / den;
      if (den < 0 && tp > 0) t = tp;
    } else if (g.type == GEOM_SPHERE) {   // _sphere_hit
      const double b = dot3(d, g.oa);
      const double h = b * b - g.cca;
      const double ts = -b - sqrt(h > 0 ? h : 0.0);
      if (h > 0 && ts > 0) t = ts;
    } else if (g.type == GEOM_CAPSULE) {   // _capsule_hit: the cylinder, then the cap of the end it fell past
      const double bard = dot3(d, g.ba), rdoa = dot3(d, g.oa);
      const double k2 = g.baba - bard * bard;
      const double k1 = g.baba * rdoa - g.baoa * bard;
      const double h = k1 * k1 - k2 * g.k0;
      const bool ok = h >= 0;
      // k2 == 0 (a ray along the axis): tc is +-inf or NaN, every comparison below is then false or
      // picks the far cap -- some pixel value, no trap (fp64 division by zero does not fault here)
      const double tc = (-k1 - sqrt(ok ? h : 0.0)) / k2;
      const double yy = g.baoa + tc * bard;
      const bool body = ok && yy > 0 && yy < g.baba && tc > 0;
      if (body) t = tc;
      const bool enda = yy <= 0;
      const double bb = dot3(d, enda ? g.oa : g.ob);
      const double hh = bb * bb - (enda ? g.cca : g.ccb);
      const double tcap = -bb - sqrt(hh > 0 ? hh : 0.0);
      if (ok && !body && hh > 0 && tcap > 0) t = tcap;
    }
    if (t < tbest) {
      tbest = t;
      gid = gi;
    }
  }

  // -- shading (Renderer._shade) ---------------------------------------------------------------------
  double out[3];
  if (gid < 0) {
    const double sky = 0.5 * (d[2] + 1);
    for (int k = 0; k < 3; k++) out[k] = sky * SKY_TOP[k];
  } else {
    const SceneGeom& g = s.g[gid];
    double p[3], nrm[3], col[3];
    for (int k = 0; k < 3; k++) p[k] = s.cpos[k] + tbest * d[k];
    if (g.type == GEOM_PLANE) {
      const double c = floor(p[0] / 0.5) + floor(p[1] / 0.5);
      const int odd = c * 0.5 != floor(c * 0.5);   // (int)c & 1, two's complement (huge |c| is even)
      for (int k = 0; k < 3; k++) {
        nrm[k] = g.ax[k];
        col[k] = FLOOR_RGB[odd][k];
      }
    } else {
      double pa[3], nn[3];
      for (int k = 0; k < 3; k++) pa[k] = p[k] - g.a[k];
      const double sc_ax = fmin(fmax(dot3(pa, g.ax), 0.0), g.hl2);
      for (int k = 0; k < 3; k++) nn[k] = p[k] - (g.a[k] + sc_ax * g.ax[k]);
      const double len = fmax(sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]), 1e-12);
      for (int k = 0; k < 3; k++) {
        nrm[k] = nn[k] / len;
        col[k] = BODY_RGB[k];
      }
    }
    const double head = clip01(-dot3(nrm, d));
    double ld[3];
    for (int k = 0; k < 3; k++) ld[k] = s.light[k] - p[k];
    const double ll = sqrt(ld[0] * ld[0] + ld[1] * ld[1] + ld[2] * ld[2]);
    for (int k = 0; k < 3; k++) ld[k] = ld[k] / ll;
    const double top = clip01(dot3(nrm, ld));
    const double lit = 0.35 + 0.45 * head + 0.35 * top;
    for (int k = 0; k < 3; k++) out[k] = col[k] * lit;
  }
  if (x >= W || y >= H) return;   // edge tiles: past every barrier, only the store is skipped
  uint8_t* px = rgb + ((frame * (size_t)H + (size_t)y) * (size_t)W + (size_t)x) * 3;
  for (int k = 0; k < 3; k++) px[k] = (uint8_t)(int)(clip01(out[k]) * 255 + 0.5);
}

}  // namespace

template <typename T>
hipError_t launch_render(const T* kin, int n, const RenderScene& scene, const RenderCam& cam, int H, int W,
                         uint8_t* rgb, hipStream_t stream) {
  if (n < 1 || H < 1 || W < 1 || scene.ngeom < 0 || scene.ngeom > MAXGEOM) return hipErrorInvalidValue;
  constexpr int MAXZ = 65535;   // gridDim.z
  const size_t frame_bytes = (size_t)H * (size_t)W * 3;
  for (int f0 = 0; f0 < n; f0 += MAXZ) {
    const int nf = std::min(MAXZ, n - f0);
    const dim3 grid((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, nf);
    hipLaunchKernelGGL((render_kernel<T>), grid, dim3(TILE * TILE), 0, stream, kin + (size_t)f0 * KINDIM, scene, cam,
                       H, W, rgb + (size_t)f0 * frame_bytes);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template hipError_t launch_render<float>(const float*, int, const RenderScene&, const RenderCam&, int, int, uint8_t*,
                                         hipStream_t);
template hipError_t launch_render<double>(const double*, int, const RenderScene&, const RenderCam&, int, int, uint8_t*,
                                          hipStream_t);

}  // namespace hs
