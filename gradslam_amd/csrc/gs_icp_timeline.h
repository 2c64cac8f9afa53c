// gs_icp_timeline.h — debugging aids of the ICP loop (gs_icp_loop.hip includes this behind its kernels): the host side of
// the per-block time stamps the kernels record in a library built with -DGS_ICP_TIMELINE.
#pragma once

// tools/icp_timeline.py: per-block time stamps of ONE iteration's two launches
// (GRADSLAM_HIP_ICP_TIMELINE_IT; default: the last), the first half into <path>, the look-ahead that follows it back to
// back into <path>.next (their first block starts are one launch period apart); both are written after the second launch.
constexpr size_t ICP_TL_HALF = 72 * 7000;   // words per launch: 72 per block
static unsigned long long* g_icp_tl_buf = nullptr;
// the record buffer of this launch (NULL: not recorded); the first half clears the buffer of both
static unsigned long long* icp_tl_arm(bool full, int nblocks, int it, int numiters, hipStream_t st) {
  const GsEnv& env = gs_env();
  if (!env.icp_timeline || it != env.timeline_it(numiters)) return nullptr;
  unsigned long long*& buf = g_icp_tl_buf;
  if (!buf && hipMalloc(&buf, 8 * 2 * ICP_TL_HALF) != hipSuccess) buf = nullptr;
  if (!buf || 72 * (size_t)nblocks > ICP_TL_HALF) return nullptr;
  if (full) (void)hipMemsetAsync(buf, 0, 8 * 2 * ICP_TL_HALF, st);
  return buf + (full ? 0 : ICP_TL_HALF);
}
// behind the look-ahead launch: synchronous dump of the two launches' block records
static void icp_tl_dump(const IcpHalfBatch& hb, const IcpHalfPlan& pl, int lmode, hipStream_t st) {
  std::unique_ptr<unsigned long long[]> h(new unsigned long long[2 * ICP_TL_HALF]);
  if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(h.get(), g_icp_tl_buf, 8 * 2 * ICP_TL_HALF, hipMemcpyDeviceToHost) != hipSuccess) return;
  for (int part = 0; part < 2; ++part) {
    char path[1024];
    snprintf(path, sizeof(path), "%s%s", gs_env().icp_timeline, part ? ".next" : "");
    FILE* f = fopen(path, "w");
    if (!f) continue;
    fprintf(f, "# B=%d G=%d nb=%d upb=%d lmode=%d: block start end(100MHz ticks) hw_id xcc_id after_prologue after_search after_unres n_unres\n", hb.B, pl.G, pl.nb, pl.upb, lmode);
    for (size_t i = 0; i < (size_t)hb.B * pl.nb; ++i) {
      fprintf(f, "%zu", i);
      for (int k = 0; k < 72; ++k) fprintf(f, " %llu", h[part * ICP_TL_HALF + 72 * i + k]);
      fprintf(f, "\n");
    }
    fclose(f);
  }
}
