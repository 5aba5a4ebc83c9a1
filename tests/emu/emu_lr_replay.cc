// emu_lr_replay.cc -- TEST INFRASTRUCTURE ONLY (tests/test_lr_replay_emu.py compiles it on its own, once plain and once with -DLANCET_FAT=1;
// the Makefile's libraries do not hold it).
//
// The --linked-reads replay alone, on hand-made csr runs: what loadSequence does to one node's barcode sets and haplotype counters
// (reference src/Graph.cc:239-317, src/Node.cc:30-118, 502-520) as kernels.h states it twice -- lr_node_replay (one lane, 16-bit fields)
// and lr_replay_batches (the whole wave, 8-bit fields, LDS batches) -- each from the same start state, on a work space that holds just
// what they touch.  The plain model they are held against is tests/test_lr_replay_emu.py's: strings and sets, no code shared.
#define LANCET_WAVE_EMU 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#ifndef LANCET_EMU_KERNELS_H
#define LANCET_EMU_KERNELS_H "../../lancet_amd/csrc/kernels.h"
#endif
#include LANCET_EMU_KERNELS_H

namespace {
struct Input {
  uint32_t n_nodes; const uint32_t *nocc, *o_read, *o_pos, *o_st; uint32_t R; const uint32_t *rinfo, *bx_rank; const uint8_t *hp;
};
enum { NODE_WORDS = 12, OCC_WORDS = 3, G0 = 5 };       // the window's reads begin at read G0 of the batch: what lies before them is not theirs

struct Rig {
  lancet_params P; EngineCaps C; DevBatch B; Work W; WinShared S; Ctx c;
  std::vector<cs_t> csr; std::vector<uint32_t> mv, scratch, rinfo, bx, read_begin; std::vector<uint8_t> hp; std::vector<NodeGr> gr; std::vector<uint16_t> khp;
  uint32_t total;
  explicit Rig(const Input &in) : total(in.nocc[in.n_nodes]) {
    memset(&P, 0, sizeof(P)); memset(&C, 0, sizeof(C)); memset(&B, 0, sizeof(B)); memset(&W, 0, sizeof(W)); memset(&S, 0, sizeof(S));
    csr.resize(total + 8); mv.assign(total + 8, 0xA5A5A5A5u); scratch.assign(2 * (size_t)in.n_nodes + 64, 0xA5A5A5A5u);
    for (uint32_t i = 0; i < total; ++i) csr[i] = CS_MAKE(in.o_read[i], in.o_pos[i], (in.o_read[i] + in.o_pos[i]) & 1u, in.o_st[i]);      // (an orientation bit, to see it kept)
    // reads of another window in front: tumour, forward, barcode 0, haplotype 1 -- a replay that forgot read_begin would count them
    rinfo.assign(G0, 100u); bx.assign(G0, 0u); hp.assign(G0, 1);
    rinfo.insert(rinfo.end(), in.rinfo, in.rinfo + in.R); bx.insert(bx.end(), in.bx_rank, in.bx_rank + in.R); hp.insert(hp.end(), in.hp, in.hp + in.R);
    read_begin = {0u, (uint32_t)G0, (uint32_t)G0 + in.R};
    gr.resize(in.n_nodes); memset(gr.data(), 0xEE, gr.size() * sizeof(NodeGr)); khp.assign(6 * (size_t)in.n_nodes, 0xEEEE);
    B.read_begin = read_begin.data(); B.rinfo = rinfo.data(); B.bx_rank = bx.data(); B.hp = hp.data();
    W.csr = (uint32_t *)csr.data(); W.mv = mv.data(); W.scratch = scratch.data(); W.gr = gr.data(); W.khp = khp.data();
    S.w = 1; S.R = (int)in.R; S.LR = 1; S.QS = 10;
    c.P = &P; c.B = &B; c.C = &C; c.W = &W; c.OUT = nullptr; c.S = &S;
  }
  void dump_runs(const Input &in, uint32_t *o) const {
    for (uint32_t i = 0; i < total; ++i, o += OCC_WORDS) { const cs_t e = csr[i]; o[0] = CS_READ(e); o[1] = CS_POS(e); o[2] = CS_ST(e) | (((uint32_t)e >> 29) << 8) | (CS_ORI(e) << 16); }
    (void)in;
  }
};

// driver 0: one lane per node
void run_lane(const Input &in, uint32_t *out) {
  Rig r(in);
  for (uint32_t n = 0; n < in.n_nodes; ++n) {
    uint32_t *o = out + (size_t)NODE_WORDS * n, v[10];
    lr_node_replay(r.c, in.nocc[n], in.nocc[n + 1], v);
    for (int q = 0; q < 10; ++q) o[q] = v[q];
    o[10] = v[0] + v[1] + v[2] + v[3]; o[11] = 0;
  }
  r.dump_runs(in, out + (size_t)NODE_WORDS * in.n_nodes);
}

// drivers 1, 2: the list as build_gather and load_prebuilt_lr make it (a node of LR_COOP_MIN..LR_COOP_MAX occurrences is listed, any other
// one replayed on the spot), then the wave
void run_wave(const Input &in, uint32_t stop, uint32_t *out) {
  Rig r(in);
  r.C.debug_stop = stop;
  r.S.tmp2 = 0;
  for (uint32_t n = 0; n < in.n_nodes; ++n) {
    const uint32_t lo = in.nocc[n], hi = in.nocc[n + 1];
    uint32_t *o = out + (size_t)NODE_WORDS * n;
    if (hi - lo >= LR_COOP_MIN && hi - lo <= LR_COOP_MAX && lo < (1u << 24)) {
      const uint32_t at = (uint32_t)r.S.tmp2; r.S.tmp2 = (int)(at + 1u);
      r.scratch[2 * (size_t)at] = n; r.scratch[2 * (size_t)at + 1] = lo | ((hi - lo) << 24);
      o[11] = 1;
    } else {
      uint32_t v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      if (hi > lo) lr_node_replay(r.c, lo, hi, v);
      NodeGr &G = r.gr[n];
      for (int q = 0; q < 4; ++q) G.kc[q] = (uint16_t)v[q];
      for (int q = 0; q < 6; ++q) r.khp[6 * (size_t)n + q] = (uint16_t)v[4 + q];
      G.mincov = (int)(uint16_t)v[0] + (int)(uint16_t)v[1] + (int)(uint16_t)v[2] + (int)(uint16_t)v[3];
      o[11] = 0;
    }
  }
  lr_replay_batches(r.c, (uint32_t)r.S.tmp2);
  for (uint32_t n = 0; n < in.n_nodes; ++n) {
    uint32_t *o = out + (size_t)NODE_WORDS * n;
    for (int q = 0; q < 4; ++q) o[q] = r.gr[n].kc[q];
    for (int q = 0; q < 6; ++q) o[4 + q] = r.khp[6 * (size_t)n + q];
    o[10] = (uint32_t)r.gr[n].mincov;
  }
  r.dump_runs(in, out + (size_t)NODE_WORDS * in.n_nodes);
}
}  // namespace

// the thresholds of the list, for the cases to be placed at them
extern "C" void lancet_emu_lr_limits(uint32_t *out) { out[0] = LR_COOP_MIN; out[1] = LR_COOP_MAX; out[2] = LR_COOP_SEGS; out[3] = (uint32_t)sizeof(cs_t); }

// nocc[n_nodes + 1]: node n's run is [nocc[n], nocc[n + 1]) of (o_read, o_pos, o_st), in the order given (the order the csr pass left it in).
// Read R - 1 is the reference pseudo-read.  out: three blocks of 12 * n_nodes + 3 * total words -- driver 0 lr_node_replay, 1 lr_replay_batches,
// 2 lr_replay_batches with every run reversed on arrival.  Per node: the ten values, mincov, 1 when the wave took it; per occurrence of the run
// as left: read, position, state | grown bits << 8 | orientation << 16.
extern "C" void lancet_emu_lr_replay(uint32_t n_nodes, const uint32_t *nocc, const uint32_t *o_read, const uint32_t *o_pos, const uint32_t *o_st,
                                     uint32_t R, const uint32_t *rinfo, const uint32_t *bx_rank, const uint8_t *hp, uint32_t *out) {
  Input in; in.n_nodes = n_nodes; in.nocc = nocc; in.o_read = o_read; in.o_pos = o_pos; in.o_st = o_st; in.R = R; in.rinfo = rinfo; in.bx_rank = bx_rank; in.hp = hp;
  const size_t BW = (size_t)NODE_WORDS * n_nodes + (size_t)OCC_WORDS * nocc[n_nodes];
  run_lane(in, out);
  run_wave(in, 0u, out + BW);
  run_wave(in, 141u, out + 2 * BW);
}

#ifdef LANCET_LR_REPLAY_MAIN
// Stand-alone form for a sanitizer run on the host (g++ -fsanitize=address,undefined -DLANCET_LR_REPLAY_MAIN, with and without -DLANCET_FAT=1):
// drawn runs at the routes' and the batches' limits through all three drivers; prints a checksum, compares nothing (the test does).
int main() {
  uint32_t seed = 12345u;
  auto rnd = [&](uint32_t n) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % n; };
  const uint32_t sizes_a[] = {1, 2, 3, 4, 191, 192, 193, 300, 3, 192, 100, 92, 5, 100, 93};
  std::vector<uint32_t> sizes(sizes_a, sizes_a + sizeof(sizes_a) / sizeof(sizes_a[0]));
  for (int i = 0; i < 64; ++i) sizes.push_back(3);
  for (int i = 0; i < 130; ++i) sizes.push_back(3 + rnd(40));
  const uint32_t R = 400;
  std::vector<uint32_t> rinfo(R), bx(R), nocc(1, 0u), o_read, o_pos, o_st;
  std::vector<uint8_t> hp(R);
  for (uint32_t r = 0; r < R; ++r) { rinfo[r] = 100u | (rnd(2) << 16) | (rnd(2) << 17); bx[r] = rnd(10) < 4 ? 0xFFFFFFFFu : rnd(300); hp[r] = (uint8_t)rnd(3); }
  for (uint32_t m : sizes) {
    std::vector<uint32_t> keys;                                  // distinct (read, position), in no order
    while (keys.size() < m) { const uint32_t k = (rnd(R) << 10) | rnd(3); bool dup = false; for (uint32_t x : keys) dup = dup || x == k; if (!dup) keys.push_back(k); }
    for (uint32_t k : keys) { o_read.push_back(k >> 10); o_pos.push_back(k & 1023u); o_st.push_back(rnd(4) == 0 ? 1u + rnd(2) : 0u); }
    nocc.push_back((uint32_t)o_read.size());
  }
  const uint32_t nn = (uint32_t)sizes.size();
  std::vector<uint32_t> out(3 * ((size_t)NODE_WORDS * nn + (size_t)OCC_WORDS * nocc[nn]));
  lancet_emu_lr_replay(nn, nocc.data(), o_read.data(), o_pos.data(), o_st.data(), R, rinfo.data(), bx.data(), hp.data(), out.data());
  unsigned long long sum = 0;
  for (uint32_t x : out) sum = sum * 1099511628211ULL + x;
  printf("lr replay: %u nodes, %u occurrences, checksum %016llx\n", nn, nocc[nn], sum);
  return 0;
}
#endif
