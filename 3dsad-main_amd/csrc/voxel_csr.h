// The ordered member lists of voxel.hip (SPEC.md §20.5), shared with the feature encoder (voxel_encode.hip, SPEC.md §24).
#pragma once
#include "common.h"

namespace sad {

struct VoxLists {
    const int32_t *start;    // [B*V]: members of the voxels below s
    const int32_t *cnt;      // [B*V]: members of voxel s (uncapped)
    const int32_t *sorted;   // [members]: the rows of voxel s in ascending order at start[s] .. start[s] + cnt[s] - 1
};

// bytes of sad_voxel_workspace_bytes (a multiple of 16); sizes must have passed voxel_sizes_ok
size_t voxel_ws_bytes(int total, int B, int V);
int voxel_sizes_ok(const char *fn, long long total, int B, long long V);
// counts the members of a caller's point2voxel (numbers outside [0, V) count as -1) and builds the lists in `workspace`
void voxel_member_lists(const int32_t *p2v, const int32_t *offsets, int total, int B, int V, void *workspace, hipStream_t st,
                        VoxLists &out);

}  // namespace sad
