// TEST INFRASTRUCTURE ONLY -- the device read selection without a GPU.
// The rules (lancet_amd/csrc/select_rules.h) and the planning between the two passes (select_host.h) are the product's source; here
// LANCET_WAVE_EMU runs the lanes of every loop one after the other, the "LDS" is a struct on the heap and the table's pointers are host
// pointers.  What comes out is what lancet_engine_upload_windows leaves on the device: kept[], the window arrays and the per-read arrays.
#define LANCET_WAVE_EMU 1
#include "../../lancet_amd/csrc/select_host.h"
#include "../../lancet_amd/csrc/host_pack.h"

#include <memory>

struct SelEmu {
  int rc = 0;
  std::string reason;
  std::vector<lancet_select_summary> sum;
  std::vector<int32_t> kept, chr_id, ref_start;
  std::vector<uint32_t> read_begin, ref_off, rinfo, name_rank, base_woff, good_woff;
  std::vector<uint8_t> ref_codes;
  int need_large = 0;
};

extern "C" {

// lds_reads / lds_bases: the limits of the LDS build configuration the `need_large` count is taken against (the engine passes its own)
SelEmu *lancet_select_emu(const lancet_alignment_table *t, const lancet_window_slice *s, const lancet_host_opts *o, uint32_t lds_reads, uint32_t lds_bases) {
  SelEmu *E = new SelEmu();
  if (const char *bad = sel_table_check(t); *bad) { E->rc = LANCET_E_ARG; E->reason = std::string("lancet_alignment_table: ") + bad; return E; }      // (as lancet_device_reads_create refuses it)
  E->reason = sel_precheck(t->load_id, s, o);
  if (!E->reason.empty()) { E->rc = LANCET_NOT_TAKEN; return E; }
  const SelTable T = sel_table_of(t);
  const SelOpts O = sel_opts_of(o);
  const int n = s->n_windows;
  std::vector<SelWin> W((size_t)n);
  for (int i = 0; i < n; ++i) W[(size_t)i] = SelWin{s->start[i], s->end[i], s->chr_id[i], s->ref_off[i + 1] - s->ref_off[i]};
  E->sum.resize((size_t)n);
  std::unique_ptr<SelLds1> L1(new SelLds1());
  for (int i = 0; i < n; ++i) sel_pass1(T, W[(size_t)i], O, L1.get(), &E->sum[(size_t)i]);
  const SelPlan plan = sel_plan(s, E->sum.data(), lds_reads, lds_bases);
  E->need_large = plan.need_large;
  if (!plan.reason.empty()) { E->rc = LANCET_NOT_TAKEN; E->reason = plan.reason; return E; }
  const int nk = (int)plan.kslice.size();
  E->read_begin = plan.read_begin; E->ref_off = plan.ref_off;
  const uint32_t R = plan.read_begin[(size_t)nk];
  E->rinfo.assign(R, 0xDEADBEEFu); E->name_rank.assign(R, 0xDEADBEEFu); E->base_woff.assign(R, 0xDEADBEEFu); E->good_woff.assign(R, 0xDEADBEEFu);
  SelOut out{E->rinfo.data(), E->name_rank.data(), E->base_woff.data(), E->good_woff.data()};
  std::unique_ptr<SelLds2> L2(new SelLds2());
  for (int k = 0; k < nk; ++k) {
    const int i = plan.kslice[(size_t)k];
    E->kept.push_back(s->widx[i]); E->chr_id.push_back(s->chr_id[i]); E->ref_start.push_back(s->start[i]);
    for (uint32_t q = s->ref_off[i]; q < s->ref_off[i + 1]; ++q) E->ref_codes.push_back((uint8_t)lc_code(s->ref_bases[q]));
    const uint32_t r0 = plan.read_begin[(size_t)k];
    sel_pass2(T, W[(size_t)i], r0, plan.read_begin[(size_t)k + 1] - r0, L2.get(), out);
  }
  return E;
}
void lancet_select_emu_free(SelEmu *E) { delete E; }
int lancet_select_emu_rc(const SelEmu *E) { return E->rc; }
const char *lancet_select_emu_reason(const SelEmu *E) { return E->reason.c_str(); }
int lancet_select_emu_need_large(const SelEmu *E) { return E->need_large; }
int lancet_select_emu_caps(int *sel_cap, int *sel_hash) { *sel_cap = SEL_CAP; *sel_hash = SEL_HASH; return 0; }
// which: 0 summaries (6 u32 each), 1 kept, 2 chr_id, 3 ref_start, 4 ref_off, 5 ref_codes (bytes), 6 read_begin, 7 rinfo, 8 name_rank, 9 base_woff, 10 good_woff
const void *lancet_select_emu_array(const SelEmu *E, int which, uint64_t *bytes) {
#define ARR(v) do { *bytes = sizeof((v)[0]) * (v).size(); return (v).data(); } while (0)
  switch (which) {
    case 0: ARR(E->sum); case 1: ARR(E->kept); case 2: ARR(E->chr_id); case 3: ARR(E->ref_start); case 4: ARR(E->ref_off); case 5: ARR(E->ref_codes);
    case 6: ARR(E->read_begin); case 7: ARR(E->rinfo); case 8: ARR(E->name_rank); case 9: ARR(E->base_woff); case 10: ARR(E->good_woff);
  }
#undef ARR
  *bytes = 0; return nullptr;
}

}  // extern "C"
