// emu_settle.cc -- TEST INFRASTRUCTURE ONLY.
//
// The host emulation of the kernels with the haplotype capture (tests/hap_emu/emu_hap.cc, included as it is, which includes the emulator's
// driver tests/emu/emu_engine.cc as it is) plus the one read-back the settled windows need: which windows of a run the build kernel
// settled (layout.h PreHdr::settled), read from the hand-off headers the run left.  The emulator's driver keeps its counter block to
// itself, so the count is taken from the headers; the engine reports the build kernel's own counter (lancet_engine_settled_count).
// Settling itself is switched by LANCET_EMU_SETTLE=1 in the environment (host_common.h lc_caps_for_sizes); settle_emu.py sets it per run.
#include "../hap_emu/emu_hap.cc"

// The sizes the settled test is written for, read off the headers (read-only; settle_edge_cases.py takes its edges from here): for the
// 512-lane form (large == 0) and the 1024-lane form (large == 1)
//   out[0] gmax: survivors per group of the edge pass (build_lds_impl.h: what is left of the phase area behind the mer-table bitmap and the
//          words of the test, eight slots per survivor)
//   out[1] cap: the most survivors the test's words hold (BL_NCAP / 4 - ST_FIXED), out[2] ST_FIXED
//   out[3] PB_SCAP, out[4] PB_CCAP, out[5] BL_NCAP, out[6] LC_MAXW, out[7] BL_RMAX of the form
//   out[8] PB_QVCAP, out[9] PB_QVCAP_WIDE (quality rows of the narrow / wide hand-off: candidates * k has to fit), out[10] the table size
//          above which the 1024-lane form does not test (4096: its wide table form)
// Returns the words written.
extern "C" int lancet_settle_emu_limits(int large, uint32_t *out, int cap) {
  const uint32_t ncap = large ? (uint32_t)PB_NCAP_WIDE : (uint32_t)PB_NCAP;
  const uint32_t big = large ? (uint32_t)sizeof(bl_large::BlShared::big) : (uint32_t)sizeof(bl_small::BlShared::big);
  const uint32_t fixed = large ? bl_large::ST_FIXED : bl_small::ST_FIXED;
  const uint32_t v[11] = {(big / 4u - ncap / 32u - ncap / 4u) / 8u, ncap / 4u - fixed, fixed, (uint32_t)PB_SCAP, (uint32_t)PB_CCAP, ncap, (uint32_t)LC_MAXW,
                          large ? bl_large::LDS_READS : bl_small::LDS_READS, (uint32_t)PB_QVCAP, (uint32_t)PB_QVCAP_WIDE, 4096u};
  int n = 0;
  for (; n < 11 && n < cap; ++n) out[n] = v[n];
  return n;
}

// out[w] = PreHdr::why of window w where the build kernel turned it away (status != PB_BUILT), 0 where it built it; returns the windows, -6 as below
extern "C" int lancet_settle_emu_why(void *h, uint32_t *out, int cap) {
  const EmuResult *r = (const EmuResult *)h;
  if (r->pre.empty() || !r->pl.stride) return -6;
  const size_t nw = r->pre.size() / r->pl.stride;
  for (size_t w = 0; w < nw && (int)w < cap; ++w) {
    const PreHdr *H = (const PreHdr *)(r->pre.data() + w * r->pl.stride + PRE_OFF_HDR);
    out[w] = H->status == PB_BUILT ? 0u : H->why;
  }
  return (int)nw;
}

// out[w] = 1 for a settled window (cap >= the run's windows); returns how many there are, -6 when the run left no hand-off areas
extern "C" int lancet_settle_emu_flags(void *h, uint8_t *out, int cap) {
  const EmuResult *r = (const EmuResult *)h;
  if (r->pre.empty() || !r->pl.stride) return -6;
  const size_t nw = r->pre.size() / r->pl.stride;
  int n = 0;
  for (size_t w = 0; w < nw; ++w) {
    const PreHdr *H = (const PreHdr *)(r->pre.data() + w * r->pl.stride + PRE_OFF_HDR);
    const bool s = H->status == PB_BUILT && H->settled == 1u;
    if (s && (H->have_order != 0u || H->heavy != 0u || H->next != 0u)) return -6;      // (a settled header: no order, no hint, nothing built ahead)
    if ((int)w < cap) out[w] = s ? 1 : 0;
    if (s) ++n;
  }
  return n;
}
