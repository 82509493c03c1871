// The ONE configuration surface of libncg.so: every environment variable the library reads, with its meaning.
// (The reference has no configuration beyond constructor options; these exist for diagnosis.)
// `ncg::knob(name, default)` is the only place that calls getenv.
//
//   always honoured
//     NCG_TIMING=1        print the MSM host-finish time to stderr per call
//     NCG_NO_ENDO=1       resident bls12-381 sets never take the endomorphism MSM / GLV ladder (generic path)
//     NCG_NO_PRECOMP=1    resident sets ignore their precomputed shifted copies (per-window path)
//     NCG_MSM_C=<c>       force the MSM window width (2..16) instead of the measured table (tools/msm_csweep.py)
//     NCG_MSM_C_ENDO=<c>  the same for the endomorphism plan
//     NCG_NO_FINISH_THREADS=1   the host finish of the bls12-381 MSMs never uses its three helper threads (bls_host64.hpp FinishPool;
//                         they are created at the first MSM that can use them, sleep between MSMs, and spin for at most 0.6 ms per MSM)
//     NCG_LANE_QUEUES=<m> hardware queues of the asynchronous MSM lanes (comm.hip lane_init): 1 = streams of the top priority class, a
//                         queue pool nothing else in the process uses (default); 0 = plain streams; 2 = a full CU mask per lane stream
#pragma once
#include <cstdlib>
#include <cstring>

namespace ncg {

inline bool knob_is_public(const char* name) {
  static const char* const pub[] = {"NCG_TIMING", "NCG_NO_ENDO", "NCG_NO_PRECOMP", "NCG_MSM_C", "NCG_MSM_C_ENDO", "NCG_NO_FINISH_THREADS", "NCG_LANE_QUEUES"};
  for (const char* p : pub)
    if (std::strcmp(p, name) == 0) return true;
  return false;
}
// integer value of the variable, `dflt` when unset or not one of the public knobs above
inline int knob(const char* name, int dflt) {
  if (!knob_is_public(name)) return dflt;
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}
inline bool knob_set(const char* name) {
  if (!knob_is_public(name)) return false;
  return std::getenv(name) != nullptr;
}

}  // namespace ncg
