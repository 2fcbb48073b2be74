/*
 * equiformer_hip_dev.h -- development entry points of libequiformer_hip.so.
 *
 * NOT part of the drop-in boundary (that is equiformer_hip.h): these exist for the tests, which replay launch plans on the CPU
 * and compare production kernels bit for bit.  eqf_sfcx_dev_set changes process-global state and is not thread safe.  Nothing
 * under equiformer_amd/ calls them.  A/B measurements of kernel variants use variant builds of the library
 * (equiformer_amd/build.py --variant NAME -DEQF_...=...).
 */
#ifndef EQUIFORMER_HIP_DEV_H
#define EQUIFORMER_HIP_DEV_H

#include "equiformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* argument tables of the split-precision SeparableFCTP launches (eqf_sfcx_*) as text: kind 0 forward, 1 data gradient,
 * 2 weight gradient (one-wave kernel), 3 weight gradient (multi-wave kernel of csrc/sfcw.hip: workgroup types).  Host-only (no GPU needed): tests/test_sfcx_plan.py replays the kernels' lane-level algorithm in
 * numpy on these tables.  Returns the number of characters written or a negative error. */
int eqf_sfcx_dev_plan(int kind, const eqf_dtp_paths* paths, const eqf_irreps* out1_irreps, int n2, int E, int mode,
                      char* buf, int buflen);
/* switches of the split-precision kernels (process-global, for tests; 0 restores the default; other keys: EQF_E_BADARG):
 *   key 2   forward: 1 = always the one-wave kernel, 2 = the multi-wave kernel (csrc/sfcy.hip) wherever its planner accepts
 *   key 4   weight gradient: 1 = always the one-wave kernel, 2 = the multi-wave kernel (csrc/sfcw.hip) wherever accepted
 *   key 9   data gradient on small graphs: 1 = never split the paths of an item over two waves */
int eqf_sfcx_dev_set(int key, int value);
/* which kernel served the last launch of a family (0 forward, 1 data gradient, 2 weight gradient) of the split-precision
 * entry points; the call clears the record (0: no launch of that family since the last call; other families: EQF_E_BADARG).
 * Host statics written beside the launch: no kernel is launched and no launch changes.
 *   forward          1 / 2 / 4 = one-wave kernel, that many waves per item; 8 = multi-wave kernel (csrc/sfcy.hip)
 *   data gradient    1 = one wave per item, 2 = paths of an item split over two waves, 3 = degree-3 layout (two half passes)
 *   weight gradient  1 = one-wave kernel, 2 = multi-wave kernel (csrc/sfcw.hip) */
int eqf_sfcx_dev_served(int family);

#ifdef __cplusplus
}
#endif
#endif /* EQUIFORMER_HIP_DEV_H */
