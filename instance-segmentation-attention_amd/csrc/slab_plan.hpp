// The grid of a weight-gradient launch that writes one partial slab set per workgroup in x.  Host arithmetic only (no
// HIP include): a wrong answer here is an out-of-bounds slab store, so it lives once, where a CPU test reaches it
// (tests/test_slab_plan.py).
#pragma once
#include "../../include/isa_kernels.h"

// grid of a grouped launch: a multiple of G, at least G
static inline long group_grid(long gx, int G) { if (G <= 1) return gx < 1 ? 1 : gx; gx = gx / G * G; return gx < G ? G : gx; }

// want: the workgroups in x the caller would like (its own occupancy formula); set_floats: what ONE of them writes (for
// every y and z of the grid); ws_floats: the workspace.  A workspace that does not hold one set per statistic group is
// refused: ISA_ENOMEM when it is what an arena has left, ISA_EINVAL when it is the caller's.  Otherwise *gx is a multiple
// of G with G <= *gx and *gx * set_floats <= ws_floats.
static inline int slab_grid(long want, long set_floats, long ws_floats, int G, bool arena, long* gx) {
    if (G < 1) G = 1;
    const long ws_cap = set_floats > 0 ? ws_floats / set_floats : 0;
    if (ws_cap < G) return arena ? ISA_ENOMEM : ISA_EINVAL;
    if (want < 1) want = 1;
    *gx = group_grid(want < ws_cap ? want : ws_cap, G);
    return ISA_OK;
}
