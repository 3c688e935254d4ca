// Launch plan of the three-step pass (k_three_stage7_lds): which workgroup computes which z chunk of which tile column.
// Host-only arithmetic on plain ints -- no HIP types, so that a C++ compiler checks it alone (tests/test_ts3_plan.py); the struct is
// passed to the kernel by value and decoded there on the scalar unit.
//
// A tile column is one (tx, ty) tile of the x-y tiling, numbered ty * ntx + tx; a workgroup marches one column through one chunk of
// planes.  A plan is an ordered list of at most three segments.  A segment takes a contiguous range of columns and a z range, cuts
// the z range into layers of `zc` planes (the last one may be shorter) and owns the blocks first .. first + ncol * nl - 1, layer by
// layer: block first + p * ncol + r is column col0 + r of the layer at position p.  Position p is layer p (natural order) or, with
// interleaved halves, layers 0, h, 1, h + 1, .. with h = (nl + 1) / 2: two layers per round of the CUs then walk up the lower and
// the upper half of the box, and the chunk above a finished one starts right after it, while its halo planes are still cached.
//
// The one-segment plan is the uniform grid the pass has always had.  The whole-round plan makes the main segment ncol = P / m
// columns wide, so that m layers are exactly one round of P workgroups (one workgroup per CU) and m * R layers R rounds with no
// partly filled round; the columns that do not fit go to a trailing segment of many short chunks, which the CUs pick up as they
// come free.
#pragma once

namespace examg {

constexpr int TS3_MAX_SEG = 3;
constexpr int TS3_NATURAL = 0, TS3_INTERLEAVED = 1;

struct TS3Seg {
  int col0, ncol;      // tile columns col0 .. col0 + ncol - 1
  int z0, z1;          // output planes z0 .. z1 - 1, relative to the first plane of the box
  int zc;              // planes per chunk
  int nl;              // layers: (z1 - z0 + zc - 1) / zc
  int first;           // first block index; an unused segment has first = nblocks
  int order;           // TS3_NATURAL or TS3_INTERLEAVED
};

struct TS3Plan {
  int nseg, nblocks;
  TS3Seg seg[TS3_MAX_SEG];
};

// plane steps of a chunk of zc planes: zc + 4 steps in whole groups of four, and the prologue's four planes
inline int ts3_chunk_cost(int zc) { return ((zc + 7) & ~3) + 4; }

// layer of the segment at position p of its block order
inline int ts3_layer_at(const TS3Seg &s, int p) {
  if (s.order != TS3_INTERLEAVED) return p;
  return (p & 1) ? (s.nl + 1) / 2 + (p >> 1) : (p >> 1);
}

inline void ts3_plan_clear(TS3Plan &pl) {
  pl.nseg = 0;
  pl.nblocks = 0;
  for (int i = 0; i < TS3_MAX_SEG; ++i) pl.seg[i] = TS3Seg{0, 0, 0, 0, 4, 0, 0, TS3_NATURAL};
}

// append a segment (nothing is appended for an empty range of columns or planes); ts3_plan_close fixes the unused ones
inline void ts3_plan_add(TS3Plan &pl, int col0, int ncol, int z0, int z1, int zc, int order) {
  if (ncol <= 0 || z1 <= z0 || pl.nseg >= TS3_MAX_SEG) return;
  if (zc < 1) zc = 1;
  if (zc > z1 - z0) zc = z1 - z0;
  TS3Seg &s = pl.seg[pl.nseg++];
  s.col0 = col0; s.ncol = ncol; s.z0 = z0; s.z1 = z1; s.zc = zc;
  s.nl = (z1 - z0 + zc - 1) / zc;
  s.first = pl.nblocks;
  s.order = s.nl > 2 ? order : TS3_NATURAL;
  pl.nblocks += ncol * s.nl;
}

inline void ts3_plan_close(TS3Plan &pl) {
  for (int i = pl.nseg; i < TS3_MAX_SEG; ++i) pl.seg[i].first = pl.nblocks;
}

// the uniform grid: every column, chunks of zc planes, layers in their natural order
inline TS3Plan ts3_plan_uniform(int C, int planes, int zc) {
  TS3Plan pl;
  ts3_plan_clear(pl);
  ts3_plan_add(pl, 0, C, 0, planes, zc, TS3_NATURAL);
  ts3_plan_close(pl);
  return pl;
}

// planes per chunk of the uniform grid: the chunk count that minimises rounds of P workgroups x plane steps of a chunk, chunks of
// 16 .. cmax planes where the box has them
inline int ts3_uniform_zc(int C, int planes, int P, int cmax, long long *cost_out = nullptr) {
  int zc = planes;
  long long best = -1;
  for (int t = 1; t <= (planes + 7) / 8; ++t) {
    const int c = (planes + t - 1) / t, tt = (planes + c - 1) / c;
    if ((c > cmax && t < (planes + 7) / 8) || (c < 16 && t > 1)) continue;
    const long long cost = (((long long)C * tt + P - 1) / P) * ts3_chunk_cost(c);
    if (best < 0 || cost < best) { best = cost; zc = c; }
  }
  if (zc + 3 < planes) zc = (zc + 3) & ~3;       // zc + 4 steps: a multiple of four wastes none
  if (cost_out) *cost_out = best;
  return zc;
}

// layers per round of the whole-round plan: the smallest m with P / m <= C columns in the main segment (1 where the box has more
// columns than the device CUs: a main segment of P columns)
inline int ts3_layers_per_round(int C, int P) {
  if (C < 1 || P < 1) return 0;
  int m = 1;
  while (P / m > C) ++m;
  return m;
}

// The whole-round plan with m layers per round and R rounds: the first P / m columns in m * R layers, the others in at least P chunks of
// a few planes.  Chunk lengths are multiples of four.
inline TS3Plan ts3_plan_rounds(int C, int planes, int P, int m, int R, int order) {
  TS3Plan pl;
  ts3_plan_clear(pl);
  if (m < 1) m = 1;
  if (R < 1) R = 1;
  int cm = P / m;
  if (cm < 1) cm = 1;
  if (cm > C) cm = C;
  const int k = m * R;
  int zc = ((planes + k - 1) / k + 3) & ~3;
  ts3_plan_add(pl, 0, cm, 0, planes, zc, order);
  const int left = C - cm;
  if (left > 0) {
    const int per_col = (P + left - 1) / left;
    int lzc = ((planes + per_col - 1) / per_col + 3) & ~3;
    if (lzc < 4) lzc = 4;
    ts3_plan_add(pl, cm, left, 0, planes, lzc, TS3_NATURAL);
  }
  ts3_plan_close(pl);
  return pl;
}

// makespan of a plan in plane steps on P CUs: segment after segment, whole rounds each
inline long long ts3_plan_cost(const TS3Plan &pl, int P) {
  long long cost = 0;
  for (int i = 0; i < pl.nseg; ++i)
    cost += (((long long)pl.seg[i].ncol * pl.seg[i].nl + P - 1) / P) * ts3_chunk_cost(pl.seg[i].zc);
  return cost;
}

// rounds of the whole-round plan: the fewest plane steps with main chunks of minzc .. cmax planes (0: none fits)
inline int ts3_best_rounds(int C, int planes, int P, int m, int minzc, int cmax, long long *cost_out = nullptr) {
  int bestR = 0;
  long long best = -1;
  for (int R = 1; R * m <= (planes + 3) / 4; ++R) {
    const TS3Plan pl = ts3_plan_rounds(C, planes, P, m, R, TS3_NATURAL);
    const int zc = pl.seg[0].zc;
    if (zc > cmax) continue;
    if (zc < minzc && R > 1) break;
    const long long cost = ts3_plan_cost(pl, P);
    if (best < 0 || cost < best) { best = cost; bestR = R; }
  }
  if (cost_out) *cost_out = best;
  return bestR;
}

struct TS3Rule {
  int P;               // CUs: one workgroup each
  int cmax;            // longest chunk of the uniform grid
  int rounds_cmax;     // longest main chunk of the whole-round plan (<= 0: never the whole-round plan)
  int order;           // layer order of its main segment
  int force_zc;        // > 0: the uniform grid with chunks of that many planes
  int force_m, force_rounds;   // > 0 either: the whole-round plan with that many layers per round / rounds (the other by the rule)
};

// The launcher's rule.  A forced chunk length gives the uniform grid; otherwise the whole-round plan where it takes fewer plane steps
// than the uniform grid of ts3_uniform_zc and at most a sixteenth of the columns is left over (the short chunks of the trailing
// segment fetch two to three times the planes they produce: 512^3 leaves 2 of 130 columns, 1024^3 would leave 212 of 468 and keeps
// the uniform grid, as every box of many more columns than CUs does).
inline TS3Plan ts3_plan(int C, int planes, const TS3Rule &r) {
  if (r.force_zc > 0) return ts3_plan_uniform(C, planes, r.force_zc < planes ? r.force_zc : planes);
  const int P = r.P > 0 ? r.P : 1;
  const bool forced = r.force_m > 0 || r.force_rounds > 0;
  long long ucost = 0;
  const int uzc = ts3_uniform_zc(C, planes, P, r.cmax, &ucost);
  const int m = r.force_m > 0 ? r.force_m : ts3_layers_per_round(C, P);
  const bool few_left = m > 0 && (long long)(C - (P / m < C ? P / m : C)) * 16 <= C;
  if (m > 0 && (forced || (r.rounds_cmax > 0 && few_left))) {
    long long rcost = 0;
    const int R = r.force_rounds > 0 ? r.force_rounds : ts3_best_rounds(C, planes, P, m, 16, forced && r.rounds_cmax <= 0 ? planes : r.rounds_cmax, &rcost);
    if (R > 0 && (forced || rcost < ucost)) return ts3_plan_rounds(C, planes, P, m, R, r.order);
  }
  return ts3_plan_uniform(C, planes, uzc);
}

}  // namespace examg
