// gs_icp_timeline.h — debugging aids of the ICP loop (gs_icp_loop.hip includes this behind its kernels): the host side of
// the per-block time stamps the kernels record in a library built with -DGS_ICP_TIMELINE.
#pragma once

// ---- the launch-per-half-iteration path (tools/icp_timeline.py): per-block time stamps of ONE iteration's two launches
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

#ifdef GS_ICP_TIMELINE
// ---- the persistent solve (GRADSLAM_HIP_ICP_PERSIST_TIMELINE=<path>; tools/icp_persist_timeline.py): per block, the
// phase stamps of ONE iteration's two half-iterations
constexpr size_t PS_TL_WORDS = 72 * (size_t)GS_XCDS * PS_CUS_PER_XCD;
static unsigned long long* g_ps_tl_buf = nullptr;
// in front of the persistent launch: sets pb.timeline / pb.tl_h
static void ps_tl_arm(IcpPersistBatch& pb, int numiters, hipStream_t st) {
  if (!gs_env().icp_persist_timeline) return;
  if (!g_ps_tl_buf && hipMalloc(&g_ps_tl_buf, 8 * PS_TL_WORDS) != hipSuccess) g_ps_tl_buf = nullptr;
  if (!g_ps_tl_buf) return;
  (void)hipMemsetAsync(g_ps_tl_buf, 0, 8 * PS_TL_WORDS, st);
  pb.timeline = g_ps_tl_buf;
  pb.tl_h = 2 * gs_env().timeline_it(numiters);
}
// behind it: synchronous dump
static void ps_tl_dump(const IcpPersistBatch& pb, hipStream_t st) {
  if (!pb.timeline) return;
  std::unique_ptr<unsigned long long[]> hbuf(new unsigned long long[PS_TL_WORDS]);
  if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(hbuf.get(), g_ps_tl_buf, 8 * PS_TL_WORDS, hipMemcpyDeviceToHost) != hipSuccess) return;
  FILE* f = fopen(gs_env().icp_persist_timeline, "w");
  if (!f) return;
  fprintf(f, "# B=%d nb=%d upb=%d h0=%d tl_h=%d: per block: xcc lb end | first half: wait_done sums scalar check rare arrived at_barrier research hard brute - - | look-ahead: the same | start releases... (100 MHz ticks)\n",
          pb.B, pb.nb, pb.upb, pb.h0, pb.tl_h);
  for (size_t i = 0; i < PS_TL_WORDS / 72; ++i) {
    const unsigned long long* r = hbuf.get() + 72 * i;
    if (!r[0]) continue;
    fprintf(f, "%llu %llu %llu |", r[1], r[2], r[3]);
    for (int k = 8; k < 32; ++k) fprintf(f, " %llu%s", r[k], k == 19 ? " |" : "");
    fprintf(f, " | %llu", r[4]);   // block start, then the release time of every half-iteration, then the end
    for (int k = 32; k < 72; ++k) fprintf(f, " %llu", r[k]);
    fprintf(f, "\n");
  }
  fclose(f);
}
#endif
