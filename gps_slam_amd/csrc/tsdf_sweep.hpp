// The ordered sweep over the hash slots (defined in tsdf_fusion.hip): the list of the slots that satisfy a predicate, in ascending
// slot order, without a host round trip -- count per SWEEP_SLOTS slots, single-workgroup scan of the counts, write.  Three launches.
#pragma once
#include "tsdf_common.hpp"

namespace gpst {

enum SlotPredicate {
    SLOT_VISIBLE_LIVE = 0,  // the live frame's visible list (types 1/2 stay, type 3 is re-tested against the frustum of M); UPDATES
                            // visible_type and folds the allocation's bookkeeping into the counters
    SLOT_VISIBLE_FREE = 1,  // every allocated block inside the frustum of M
    SLOT_ALLOCATED = 2,     // every allocated block (ptr >= 0); M is not read
};

// One scene (views == NULL): the slots of `s` that satisfy `pred` go to list[0 .. min(*count, cap)), their number -- not clamped
// -- to *count (device addresses); counts [sweep_blocks(s)] and flags [n_buckets + n_excess bytes] are the sweep's scratch.
// n views of one scene (views = the device table of n records, grid.z = view): SLOT_VISIBLE_FREE with each record's pose and
// intrinsics, into the record's visible_ids / counters[GPS_TSDF_N_VISIBLE_FREE], through the record's own scratch; M, counts,
// flags, list and count are not read.
// -> GPS_OK or GPS_ERR_LAUNCH
int sweep_slots(const TsdfState& s, SlotPredicate pred, const Mat4& M, int32_t* counts, uint8_t* flags, int32_t* list, int cap,
                int32_t* count, int n_views, const ViewRec* views, hipStream_t st);

}  // namespace gpst
