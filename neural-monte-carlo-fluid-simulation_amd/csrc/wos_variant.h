// wos_variant.h -- which instantiation of wos_first_ball_kernel and wos_walk_kernel a solve
// runs.  Host only (plain C++ over wos_scene.h): kernel_variant() is the one place that
// reads the scene and the parameters for that choice; the launchers and the occupancy
// query (wos_launch.h) take its result, and wos_select.h maps it to a kernel.
#pragma once
#include "wos_scene.h"

namespace wos {

// The template arguments of the two kernels, as values:
//   wos_first_ball_kernel<dim, robust, channels>
//   wos_walk_kernel<dim, geom_global, bstart, robust, neumann, spread, channels>
struct KernelVariant {
  int dim;
  bool geom_global;  // GG: geometry read from global memory instead of LDS
  bool bstart;       // BSTART: boundary-start walks (boundary value caching); no first-ball kernel
  bool robust;       // RB: robust float semantics
  bool neumann;      // NEU: the walk carries the Neumann term (false: DevParams::neumann_inert)
  bool spread;       // SPR: walks handed to idle sibling waves (DevParams::tail_spread)
  int channels;      // NC: 1 or kMaxChannels
  bool valid;        // false: no such kernel (the entry points answer hipErrorInvalidValue)
};

// Only the reference-semantics walks of a solve have Neumann-inert instantiations, and of
// those only 2D with LDS geometry has tail-spreading ones; everywhere else the two
// parameters are ignored.  Boundary-start walks exist in 2D with one channel.
inline KernelVariant kernel_variant(int dim, const DevScene& sc, const DevParams& prm, bool bstart) {
  KernelVariant v;
  v.dim = dim;
  v.geom_global = sc.geom_global != 0;
  v.bstart = bstart;
  v.robust = prm.robust != 0;
  const bool plain = !v.bstart && !v.robust;
  v.neumann = !(plain && prm.neumann_inert);
  v.spread = plain && dim == 2 && !v.geom_global && prm.tail_spread;
  v.channels = sc.n_channels > 1 ? kMaxChannels : 1;
  v.valid = (dim == 2 || dim == 3) && (!bstart || (dim == 2 && v.channels == 1));
  return v;
}

}  // namespace wos
