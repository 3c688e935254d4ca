// Stand-alone checker of the launch plans of the three-step pass (exastencils_amd/csrc/ts3_plan.h), run by tests/test_ts3_plan.py.
// For every box with C = 1 .. 600 tile columns, 20 .. 1023 planes and 8 .. 304 CUs, every plan the launcher can ask for must
//   * put every (column, plane) into exactly one chunk of exactly one segment,
//   * have chunk lengths that are multiples of four, except a segment's last chunk (rule and whole-round plans),
//   * number its blocks densely, segment after segment, with no empty segment,
//   * and, with a forced chunk length, be the uniform grid: one segment, ntz = ceil(planes / zc) layers of zc planes in natural order.
// Prints the number of plans checked; the first violation ends it with a message and exit code 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ts3_plan.h"

using namespace examg;

static long long g_checked = 0;

static void fail(const char *what, int C, int planes, int P, const char *which) {
  std::printf("FAIL: %s (C = %d, planes = %d, P = %d, %s)\n", what, C, planes, P, which);
  std::exit(1);
}

static void check(const TS3Plan &pl, int C, int planes, int P, bool mult4, const char *which) {
  ++g_checked;
  if (pl.nseg < 1 || pl.nseg > TS3_MAX_SEG) fail("segment count", C, planes, P, which);
  int next = 0;
  std::vector<int> covered(C, 0);
  std::vector<char> seen;
  for (int i = 0; i < pl.nseg; ++i) {
    const TS3Seg &s = pl.seg[i];
    if (s.ncol < 1 || s.nl < 1 || s.z1 <= s.z0) fail("empty segment", C, planes, P, which);
    if (s.col0 < 0 || s.col0 + s.ncol > C || s.z0 < 0 || s.z1 > planes) fail("segment outside the box", C, planes, P, which);
    if (s.first != next) fail("block indices not dense", C, planes, P, which);
    if (s.zc < 1 || s.nl != (s.z1 - s.z0 + s.zc - 1) / s.zc) fail("layer count", C, planes, P, which);
    if (mult4 && s.nl > 1 && (s.zc & 3)) fail("chunk length not a multiple of four", C, planes, P, which);
    if (s.order != TS3_NATURAL && s.order != TS3_INTERLEAVED) fail("layer order", C, planes, P, which);
    next += s.ncol * s.nl;
    // the positions of the block order visit every layer once; the layers tile [z0, z1) with non-empty chunks
    seen.assign(s.nl, 0);
    int planes_seen = 0;
    for (int p = 0; p < s.nl; ++p) {
      const int l = ts3_layer_at(s, p);
      if (l < 0 || l >= s.nl || seen[l]) fail("layer order is no permutation", C, planes, P, which);
      seen[l] = 1;
      const int mb = s.z0 + l * s.zc, me = mb + s.zc < s.z1 ? mb + s.zc : s.z1;
      if (me <= mb) fail("empty chunk", C, planes, P, which);
      planes_seen += me - mb;
    }
    if (planes_seen != s.z1 - s.z0) fail("chunks do not tile the z range", C, planes, P, which);
    for (int c = s.col0; c < s.col0 + s.ncol; ++c) covered[c] += s.z1 - s.z0;
    for (int j = 0; j < i; ++j) {      // rectangles of columns x planes: pairwise disjoint
      const TS3Seg &o = pl.seg[j];
      const bool cols = s.col0 < o.col0 + o.ncol && o.col0 < s.col0 + s.ncol, zs = s.z0 < o.z1 && o.z0 < s.z1;
      if (cols && zs) fail("segments overlap", C, planes, P, which);
    }
  }
  if (pl.nblocks != next) fail("block count", C, planes, P, which);
  for (int i = pl.nseg; i < TS3_MAX_SEG; ++i)
    if (pl.seg[i].first != pl.nblocks) fail("unused segment does not start past the last block", C, planes, P, which);
  for (int c = 0; c < C; ++c)
    if (covered[c] != planes) fail("a column is not covered once", C, planes, P, which);
}

// the chunk length of the uniform grid as the launcher had it before plans, restated
static int old_rule_zc(int xy, int n2, int P, int cmax) {
  int zc = n2;
  long long best = -1;
  for (int t = 1; t <= (n2 + 7) / 8; ++t) {
    const int c = (n2 + t - 1) / t, tt = (n2 + c - 1) / c;
    if ((c > cmax && t < (n2 + 7) / 8) || (c < 16 && t > 1)) continue;
    const long long cost = (((long long)xy * tt + P - 1) / P) * (((c + 4 + 3) & ~3) + 4);
    if (best < 0 || cost < best) { best = cost; zc = c; }
  }
  if (zc + 3 < n2) zc = (zc + 3) & ~3;
  return zc;
}

int main() {
  const int planes_list[] = {20, 63, 129, 255, 511, 1023}, cu_list[] = {8, 12, 104, 256, 304};
  const int forced_zc[] = {5, 16, 28, 48, 200, 2000}, rounds_cmax[] = {0, 28, 64, 128, 256, 1024};
  for (int C = 1; C <= 600; ++C)
    for (int planes : planes_list)
      for (int P : cu_list) {
        TS3Rule r{P, 64, 0, TS3_NATURAL, 0, 0, 0};
        // forced chunk length: the uniform grid
        for (int zc : forced_zc) {
          r.force_zc = zc;
          const TS3Plan pl = ts3_plan(C, planes, r);
          check(pl, C, planes, P, false, "forced zc");
          const int z = zc < planes ? zc : planes;
          if (pl.nseg != 1 || pl.seg[0].zc != z || pl.seg[0].nl != (planes + z - 1) / z || pl.seg[0].col0 != 0 || pl.seg[0].ncol != C ||
              pl.seg[0].order != TS3_NATURAL || pl.nblocks != C * ((planes + z - 1) / z))
            fail("forced zc is not the uniform grid", C, planes, P, "forced zc");
        }
        r.force_zc = 0;
        // the rule, whole rounds off and on, both orders and both chunk bounds of the uniform grid
        for (int cmax : {28, 64})
          for (int rc : rounds_cmax)
            for (int order : {TS3_NATURAL, TS3_INTERLEAVED}) {
              r.cmax = cmax;
              r.rounds_cmax = rc;
              r.order = order;
              const TS3Plan pl = ts3_plan(C, planes, r);
              check(pl, C, planes, P, true, "rule");
              if (rc == 0) {
                const int z = old_rule_zc(C, planes, P, cmax);
                if (pl.nseg != 1 || pl.seg[0].zc != (z < planes ? z : planes) || pl.seg[0].order != TS3_NATURAL)
                  fail("rule without whole rounds is not the uniform grid of the old rule", C, planes, P, "rule");
              } else if (pl.nseg > 1 || pl.seg[0].order == TS3_INTERLEAVED) {
                if (pl.seg[0].zc > rc && pl.seg[0].nl > 1) fail("main chunk longer than allowed", C, planes, P, "rule");
              }
            }
        // forced whole-round plans
        r.cmax = 64;
        r.rounds_cmax = 0;
        for (int m : {0, 1, 2, 7})
          for (int R : {0, 1, 2, 3, 4, 8, 16})
            for (int order : {TS3_NATURAL, TS3_INTERLEAVED}) {
              if (m == 0 && R == 0) continue;
              r.force_m = m;
              r.force_rounds = R;
              r.order = order;
              check(ts3_plan(C, planes, r), C, planes, P, true, "forced rounds");
            }
        r.force_m = r.force_rounds = 0;
      }
  // the headline box: 130 columns, 511 planes, 256 CUs, two layers of 128 columns per round
  {
    const TS3Plan pl = ts3_plan_rounds(130, 511, 256, 2, 4, TS3_INTERLEAVED);
    if (pl.nseg != 2 || pl.seg[0].ncol != 128 || pl.seg[0].zc != 64 || pl.seg[0].nl != 8 || pl.seg[1].col0 != 128 || pl.seg[1].ncol != 2 ||
        pl.seg[1].zc != 4 || pl.seg[1].first != 1024 || pl.nblocks != 1024 + 2 * 128 || ts3_layers_per_round(130, 256) != 2 ||
        ts3_layers_per_round(39, 256) != 7)
      fail("headline plan", 130, 511, 256, "plan A");
    const int want[8] = {0, 4, 1, 5, 2, 6, 3, 7};
    for (int p = 0; p < 8; ++p)
      if (ts3_layer_at(pl.seg[0], p) != want[p]) fail("interleaved halves", 130, 511, 256, "plan A");
  }
  std::printf("OK %lld plans\n", g_checked);
  return 0;
}
