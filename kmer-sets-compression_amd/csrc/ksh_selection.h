// A checked ksh_kss_selection as the kernels of ksh_kss_select_* (ksh_select.hip) and ksh_kss_select_class_ids
// (ksh_classids.hip) take it, and the two host checks of a request that the three calls share.
#ifndef KSH_SELECTION_H_
#define KSH_SELECTION_H_

#include "ksh_rowtile.h"

namespace ksh {

struct SelParams {
  uint64_t require[2], exclude[2];
  int32_t min_count, max_count;
};

// The predicate of a selection on the row of an occupied slot; *m = the row's popcount c(q).
__device__ __forceinline__ bool sel_judge(const SelParams& p, uint64_t r0, uint64_t r1, int* m) {
  *m = __popcll(r0) + __popcll(r1);
  return *m >= p.min_count && *m <= p.max_count && (r0 & p.require[0]) == p.require[0] &&
         (r1 & p.require[1]) == p.require[1] && ((r0 & p.exclude[0]) | (r1 & p.exclude[1])) == 0;
}

// What does not need the index: refused before it is dereferenced.
int check_request(const ksh_kss_selection* sel, const ksh_kss_index* idx);
// What reads the index's host fields: the columns, the two masks and the thresholds of a checked request.
int resolve_request(const ksh_kss_selection* sel, const IndexShape& x, pc::ColList* list, int* n_cols, SelParams* p);

}  // namespace ksh

#endif
