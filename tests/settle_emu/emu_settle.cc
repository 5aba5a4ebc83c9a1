// emu_settle.cc -- TEST INFRASTRUCTURE ONLY.
//
// The host emulation of the kernels with the haplotype capture (tests/hap_emu/emu_hap.cc, included as it is, which includes the emulator's
// driver tests/emu/emu_engine.cc as it is) plus the one read-back the settled windows need: which windows of a run the build kernel
// settled (layout.h PreHdr::settled), read from the hand-off headers the run left.  The emulator's driver keeps its counter block to
// itself, so the count is taken from the headers; the engine reports the build kernel's own counter (lancet_engine_settled_count).
// Settling itself is switched by LANCET_EMU_SETTLE=1 in the environment (host_common.h lc_caps_for_sizes); settle_emu.py sets it per run.
#include "../hap_emu/emu_hap.cc"

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
