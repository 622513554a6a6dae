// gm_check.h -- host-only argument checks of the extern "C" entry points (include/gmesh_hip.h): no device code.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/gmesh_hip.h"

namespace gm {

void set_error(const char* fmt, ...);

// One buffer of a call as a byte range.  apart: it may share no byte with any other range of the table (an output, a workspace); two
// ranges that are both not apart (read-only inputs) may alias each other.
struct ByteRange { const void* p; size_t n; const char* what; bool apart; };

// Refuses the first pair of the table (in table order) that shares memory: "fn: A overlaps B".  A NULL or empty range overlaps nothing.
// A pair the call allows to coincide (an in-place output) is the caller's business: it leaves one of the two out of the table.
static inline int check_ranges(const char* fn, const ByteRange* rg, int n) {
  for (int a = 0; a < n; a++)
    for (int b = a + 1; b < n; b++) {
      if (!rg[a].apart && !rg[b].apart) continue;
      const uintptr_t pa = reinterpret_cast<uintptr_t>(rg[a].p), pb = reinterpret_cast<uintptr_t>(rg[b].p);   // (integers: no pointer is formed past a range)
      if (!pa || !pb || !rg[a].n || !rg[b].n) continue;
      if (pa <= pb ? pb - pa < rg[a].n : pa - pb < rg[b].n) { set_error("%s: %s overlaps %s", fn, rg[a].what, rg[b].what); return GM_ERR_INVALID_ARG; }
    }
  return GM_OK;
}
template <int N>
static inline int check_ranges(const char* fn, const ByteRange (&rg)[N]) { return check_ranges(fn, rg, N); }

// the grid rules gm_tsdf_integrate, gm_surface_nets and gm_tsdf_fill share: sizes, the sample count one launch indexes, origin and voxel
#define GM_TSDF_MAX_SAMPLES (1ll << 28)
static inline int check_tsdf_grid(const char* fn, int nx, int ny, int nz, int least, const float* origin, float voxel) {
  if (nx < least || ny < least || nz < least) { set_error("%s: grid %d x %d x %d (every side at least %d)", fn, nx, ny, nz, least); return GM_ERR_INVALID_ARG; }
  if ((long long)nx * ny > GM_TSDF_MAX_SAMPLES || (long long)nx * ny * nz > GM_TSDF_MAX_SAMPLES) {
    set_error("%s: grid %d x %d x %d has more than 2^28 samples", fn, nx, ny, nz); return GM_ERR_INVALID_ARG;
  }
  if (!origin) { set_error("%s: null pointer (origin)", fn); return GM_ERR_INVALID_ARG; }
  if (!(voxel > 0.f) || voxel > 3.4028234e38f || !(origin[0] - origin[0] == 0.f) || !(origin[1] - origin[1] == 0.f) || !(origin[2] - origin[2] == 0.f)) {
    set_error("%s: voxel must be positive and finite, origin finite", fn); return GM_ERR_INVALID_ARG;
  }
  return GM_OK;
}

}  // namespace gm
