// gs_env.h — every GRADSLAM_HIP_* environment switch the library reads, in ONE place (README: the knob table).
// gs_env() reads them once per process (a function-local static: thread-safe).  None of them changes a result (tests/
// test_hip_engine_matrix.py, tests/test_hip_batch.py).  Not here: GRADSLAM_HIP_DETERMINISTIC_BACKWARD, read per call (on iff
// atoi of the value is nonzero) in two places: gs_icp_backward_f32 (gs_icp_bwd.hip) reads it itself; for the projective
// ICP's backward (gs_picp_bwd.hip) the Python layer reads it with the same rule (ops.deterministic_backward_env) and then
// calls gs_projective_icp_ordered_backward_batch_f32 -- the C entries of that file never look at the environment.
#pragma once
#include <stdlib.h>
#include <string.h>

struct GsEnv {
  // ---- engines of the batched localisation (gs_icp_loop.hip: icp_engine_plan)
  // ICP_LISTS=0: no candidate lists of ordinary queries (gs_knn.h: gl_*).
  bool icp_lists;
  // ICP_LISTS_FROM=k: the lists are built behind the look-ahead search of iteration k and tried from iteration k + 1 on
  // (unset or negative: FS_LISTS_FROM = 1).  The step of iteration 0 is the large one of a solve (millimetres); a list
  // built before it would not survive it.  Later starts were measured too: 0 / 1 / 4 / 8 give
  // 7.40 / 7.42 / 7.42 / 7.31 k frames/s at 8 sequences per GPU.
  int icp_lists_from;
  // ICP_WIDE=0: no wide lists of hard queries (gs_knn.h).
  bool icp_wide;
  // ICP_BINNED_NORMALS=0: gather the matches' normals from the map instead of the binned copy (A/B)
  bool icp_binned_normals;
  // ICP_WEAK_ROOM=<cells> (0 = off = anything outside [0, 1)): see the list-building branch of icp_half_body
  float icp_weak_room;
  // ---- launch geometry of a half-iteration (icp_half_plan; A/B runs: the results do not depend on either)
  int icp_lanes;         // ICP_LANES = 2 | 4 | 8 forces the lanes per query (0: unset)
  int icp_blocks_per_cu;   // ICP_BLOCKS_PER_CU > 0: resident-block budget per CU (experiments; else one if some G fits that, or two)
  // ---- debugging aids (library built with -DGS_ICP_TIMELINE; gs_icp_timeline.h)
  const char* icp_timeline;           // ICP_TIMELINE=<path>
  bool icp_timeline_it_set; int icp_timeline_it;   // ICP_TIMELINE_IT=k: the iteration recorded (default: the last)
  int timeline_it(int numiters) const { return icp_timeline_it_set ? icp_timeline_it : numiters - 1; }
  // ---- generic solve
  bool knn_brute;    // KNN=brute forces the brute-force engine (A/B runs; results are identical)
  int knn_spt;       // KNN_SPT = 4 | 8: source points per thread of the brute-force search (anything else: the size rule)
  bool debug_grid;   // DEBUG_GRID set: gs_localize_list_stats_i64 prints the grid header
};

inline const GsEnv& gs_env() {
  static const GsEnv env = [] {
    const auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    GsEnv v;
    v.icp_lists = num("GRADSLAM_HIP_ICP_LISTS", 1) != 0;
    v.icp_lists_from = num("GRADSLAM_HIP_ICP_LISTS_FROM", -1);
    v.icp_wide = num("GRADSLAM_HIP_ICP_WIDE", 1) != 0;
    v.icp_binned_normals = num("GRADSLAM_HIP_ICP_BINNED_NORMALS", 1) != 0;
    const char* room = getenv("GRADSLAM_HIP_ICP_WEAK_ROOM");
    v.icp_weak_room = room ? (float)atof(room) : 0.0f;
    if (!(v.icp_weak_room >= 0.0f && v.icp_weak_room < 1.0f)) v.icp_weak_room = 0.0f;
    v.icp_lanes = num("GRADSLAM_HIP_ICP_LANES", 0);
    v.icp_blocks_per_cu = num("GRADSLAM_HIP_ICP_BLOCKS_PER_CU", 0);
    v.icp_timeline = getenv("GRADSLAM_HIP_ICP_TIMELINE");
    v.icp_timeline_it_set = getenv("GRADSLAM_HIP_ICP_TIMELINE_IT") != nullptr;
    v.icp_timeline_it = num("GRADSLAM_HIP_ICP_TIMELINE_IT", 0);
    const char* knn = getenv("GRADSLAM_HIP_KNN");
    v.knn_brute = knn && strcmp(knn, "brute") == 0;
    v.knn_spt = num("GRADSLAM_HIP_KNN_SPT", 0);
    v.debug_grid = getenv("GRADSLAM_HIP_DEBUG_GRID") != nullptr;
    return v;
  }();
  return env;
}
