// What svds.hip (the truncated SVD; include/mr_lsqr.h) needs of an LSQR
// context (lsqr.hip), and what the context keeps for it.
#pragma once
#include "../../include/mr_lsqr.h"
#include "sp_structure.h"

namespace mr {

struct SvdsWork;                  // basis buffers and statistics (svds.hip)
void svds_release(SvdsWork* w);   // frees them; the context's device is current

struct SvdsHost {
  int device;
  hipStream_t s;
  const SpStructure* sp;
  LaunchTimer* timer;
  bool ptr_loads;
  mr_lsqr_stats* lstats;   // the SpMVs' timings go into K_A / K_AT
  SvdsWork** work;         // owned by the context, allocated by the first SVD
};
SvdsHost svds_host_of(mr_lsqr* ctx);   // lsqr.hip

}  // namespace mr
