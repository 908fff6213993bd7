// Run-time specialisation of the cascade kernel: generates straight-line source for a cascade's first stages
// (spec_stage_source, spec_stage_source_lbp), splices it into the text of cc_eval_kernel.inc and compiles it with hiprtc
// (loaded on demand), caching code objects in memory and on disk (spec_build, host side only), and loads the code objects
// as modules (spec_load). Switching a detector over to them is cc_detect_api.hip's (spec_install). Depends on the cascade
// model only, never on a detector.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include "cc_detect_internal.h"

namespace ccamd {

#include "build/cc_eval_kernel_src.h"  // kEvalKernelSrc: the text of cc_eval_common.h and cc_eval_kernel.inc

// Source text of spec_stage<1|2> (and spec_stage0_x2<1|2>) for the first n_stages stages: every stump becomes
// straight-line code whose LDS offsets, weights, threshold and leaf values are literals (hex floats, exact). The
// expression is the one of stump_vote(), term by term, so results are bit-identical to the table-driven path.
//
// The code is software-pipelined by construction: the LDS reads of stump i + D are issued before stump i is computed,
// and scheduling barriers pin that order (left alone, the compiler emits read, wait, compute per stump and every
// wavefront spends most of its time waiting for the LDS round trip). One copy of a stage serves the whole-stage call and
// the stump-split calls: the stage is cut into SPEC_PARTS contiguous parts, a call evaluates parts [p_lo, p_hi) and only
// its first part runs the prologue that issues the first D stumps' reads (a part's tail prefetches into the next part,
// so consecutive parts run without a pipeline drain).
struct SpecStump {
  std::string loads;    // statements "x = b[..];" (variables are declared by the caller)
  std::string decls;    // declarations of those variables
  std::string compute;  // statement adding the stump's vote to `acc`
  double base = 0.;     // constant part of the vote, added once per part (delta form, see spec_stage_source)
  long long base_q = 0; // the same in units of the stage's quantum (fixed-point form)
};

// The generated stages are called from several places of the kernel (dense group, thread phase, stump-split slices).
// Inlined everywhere, the code of every stage exists once per call site; as a real function it exists once (a third of
// the instructions for the bench cascade) at the price of the call convention's register traffic. CCAMD_SPEC_NOINLINE picks.
static const char* spec_stage_inline_attr() {
  const char* e = std::getenv("CCAMD_SPEC_NOINLINE");
  return (e && std::atoi(e) != 0) ? "__noinline__" : "__forceinline__";
}

// Emits the body of one stage from per-stump pieces (see above). `suffixes` = one accumulator / window per entry.
static void spec_emit_stage(std::string& o, const std::vector<SpecStump>& st, int depth, bool parts, const std::vector<std::string>& accs,
                            bool fixed_point = false) {
  const int nt = (int)st.size();
  static const char* kSB = "      __builtin_amdgcn_sched_barrier(0);\n";
  for (const SpecStump& t : st) o += "      " + t.decls + "\n";
  const int P = parts ? SPEC_PARTS : 1;
  char buf[128];
  int prev_nonempty = -1;  // last part before k that holds stumps
  for (int k = 0; k < P; k++) {
    const int e0 = (int)((long long)k * nt / P), e1 = (int)((long long)(k + 1) * nt / P);
    if (e0 == e1) continue;
    // The prologue (reads of the part's first `depth` stumps) belongs to the call whose range STARTS at this part -- or at
    // one of the empty parts just before it: a stage with fewer stumps than SPEC_PARTS has empty parts, and a call that
    // starts on one (the whole-stage call starts on part 0) must still issue the reads of the first stumps it evaluates.
    if (parts)
      snprintf(buf, sizeof(buf), "      if (p_lo > %d && p_lo <= %d) {\n", prev_nonempty, k);
    else
      snprintf(buf, sizeof(buf), "      {\n");
    prev_nonempty = k;
    o += buf;
    for (int i = e0; i < std::min(e0 + depth, nt); i++) o += "      " + st[(size_t)i].loads + "\n" + kSB;
    o += "      }\n";
    if (parts) {
      snprintf(buf, sizeof(buf), "      if (p_lo <= %d && %d < p_hi) {\n", k, k);
      o += buf;
    } else
      o += "      {\n";
    {  // constant parts of this part's votes (delta form): one exact addition per accumulator
      double base = 0.;
      unsigned base_q = 0;  // modulo 2^32, like the accumulator
      for (int i = e0; i < e1; i++) {
        base += st[(size_t)i].base;
        base_q += (unsigned)st[(size_t)i].base_q;
      }
      char lit[64];
      if (fixed_point)
        snprintf(lit, sizeof(lit), "%uu", base_q);
      else
        snprintf(lit, sizeof(lit), "%a", base);
      if (fixed_point ? base_q != 0 : base != 0.)
        for (const std::string& a : accs) o += "      " + a + " += " + lit + ";\n";
    }
    for (int i = e0; i < e1; i++) {
      if (depth > 0 && i + depth < nt) o += "      " + st[(size_t)(i + depth)].loads + "\n" + kSB;
      if (depth == 0) o += "      " + st[(size_t)i].loads + "\n";
      o += "      " + st[(size_t)i].compute + "\n" + kSB;
    }
    o += "      }\n";
  }
}

static std::string spec_stage_source_lbp(const Cascade& m, int n_stages, bool tile16);

// Cuts the rectangle (x, y, w, h) into the fewest strips along its longer side whose sums each fit 16 bits.
static std::vector<std::array<int, 4>> pieces16(int x, int y, int w, int h) {
  std::vector<std::array<int, 4>> out;
  const bool along_x = w >= h;
  const int len = along_x ? w : h;
  for (int k = 1; k <= std::max(len, 1); k++) {
    out.clear();
    bool ok = true;
    for (int i = 0; i < k; i++) {
      const int a = (int)((long long)i * len / k), b = (int)((long long)(i + 1) * len / k);
      if (a == b) continue;
      const std::array<int, 4> pc = along_x ? std::array<int, 4>{x + a, y, b - a, h} : std::array<int, 4>{x, y + a, w, b - a};
      ok = ok && fits16((long long)pc[2] * pc[3]);
      out.push_back(pc);
    }
    if (ok) return out;
  }
  return {};  // a single row or column of the window does not fit: the caller's eligibility test has excluded this
}

// Can the first n_stages stages be generated for STEP-2 tiles with 16-bit entries (TileGeom16)? Upright Haar features
// (any rectangle is cut into strips that fit) or LBP cells that fit; the variance rectangle is read as two halves.
static bool tile16_eligible(const Cascade& m, int n_stages) {
  // Measured in round 3. Haar: the 16-bit tile raises the resident blocks per CU from 5 to 7 and the
  // thread-per-window stages gain 4 %, but the table-driven wave phase then reads its corners from global memory and loses
  // twice that: 15 % slower as a whole -> only on request (CCAMD_SPEC_TILE16=1). LBP with EVERY stage compiled (the stock
  // cascade: 20 stages, 139 stumps) has no table-driven stage and no wave phase, and its short stages are chains of
  // dependent stump latencies that more resident wavefronts do hide: 7.6 -> 6.7 ms per 32 frames -> on by default.
  if (m.max_nodes_per_tree > 1) return false;
  const int total = (int)m.stage_ntrees.size();
  n_stages = std::min<int>(n_stages, total);
  const char* on = std::getenv("CCAMD_SPEC_TILE16");
  if (on ? std::atoi(on) == 0 : !(m.feature_type == CC_FEATURE_LBP && n_stages == total)) return false;
  if (m.feature_type == CC_FEATURE_HAAR) {
    if (m.has_tilted) return false;
    const int nrx = m.win_w - 2, nry = m.win_h - 2;
    if (nrx < 2 || !fits16((long long)(nrx - (nrx >> 1)) * nry)) return false;
    if (!fits16(std::max(m.win_w, m.win_h))) return false;  // strips of one row / column always fit
    return true;
  }
  for (int s = 0; s < n_stages; s++)
    for (int i = 0; i < m.stage_ntrees[(size_t)s]; i++) {
      const int32_t* r = &m.lbp_rects[(size_t)m.stump_feature[(size_t)m.stage_first[(size_t)s] + i] * 4];
      if (!fits16((long long)r[2] * r[3])) return false;
    }
  return true;
}

static std::string spec_stage_source(const Cascade& m, int n_stages, int tmode) {
  const CNumericLocale c_numbers;  // "%a" literals must not follow the host program's LC_NUMERIC
  if (m.feature_type == CC_FEATURE_LBP) return spec_stage_source_lbp(m, n_stages, tmode == TILE_16);
  std::vector<HaarStumpDev> t[2];
  build_haar_stumps<1>(m, t[0]);
  build_haar_stumps<2>(m, t[1]);
  const TileGeom16 G16(m.win_w, m.win_h);
  n_stages = std::min<int>(n_stages, (int)m.stage_ntrees.size());
  const int depth = 2;  // stumps whose reads are issued ahead of the one being computed
  // Delta form of a vote: `(v < thr ? left : right)` needs both leaf values in registers (a select takes one literal), and
  // the compiler hoists those ~2 registers per stump out of the stage loop until it spills; `right + (v < thr ? left - right
  // : 0)` selects between ONE literal and zero, and the `right`s of a part add up to one constant. Exact -- hence equal to
  // the sequential sum of the votes -- when every partial sum of leaves and differences is representable
  // (stage_sums_order_independent with headroom for the differences); otherwise the plain form is generated.
  const bool delta_form = stage_sums_order_independent(m, 4.0);
  std::string o;
  char buf[512];
  auto hexf = [&](float v) {
    snprintf(buf, sizeof(buf), "%af", (double)v);
    return std::string(buf);
  };
  // One stump. When every weight is a small integer and sum |w_j| * 255 * area_j < 2^24, every intermediate of the
  // float expression w0*(float)r0 + w1*(float)r1 [+ w2*(float)r2] is an exactly representable integer, so the value
  // equals (float) of the same combination computed in int32: corners shared by the rectangles merge, one conversion
  // instead of three, no float multiplies. Otherwise the float expression is emitted term by term.
  // `win` names the window (variables x<stump>_<k><win>, base pointer b<win>, vnf<win>, acc<win>).
  // Fixed-point votes. Where a stage's leaves are all multiples of q = 2^k and the sum of their magnitudes stays below
  // 2^31 q, the stage sum of ANY subset of votes is an int32 multiple of q: the delta-form votes are then accumulated as
  // 32-bit integers (one select + one add per stump instead of two selects and a double add; intermediate wrap-around
  // is harmless modulo 2^32) and converted once, exactly, at the end: (double)(int)acc * q is the same real number the
  // double accumulation produces, so every comparison and reported sum is bit-identical.
  std::function<std::string(const HaarStumpDev&, const std::string&, double, SpecStump&)> vote_text;
  // `reuse`: words the stump evaluated just before this one holds in variables (tile offset -> name): a corner both stumps
  // read is not loaded again. `vars_out` receives this stump's own map for the next one.
  auto stump = [&](const HaarStumpDev& d, int stump_index, int local, const std::string& win, double fixed_q, bool h16,
                   const std::map<int, std::string>* reuse = nullptr, std::map<int, std::string>* vars_out = nullptr) {
    const int fi = m.stump_feature[(size_t)stump_index];
    const std::string tile_ptr = (h16 ? "h" : "b") + win;  // h<win>: the same tile base as 16-bit entries
    bool int_ok = true;
    double bound = 0;
    for (int j = 0; j < d.nrect; j++) {
      const float w = d.w[j];
      const int32_t* r = &m.haar_rects[(size_t)fi * 12 + j * 4];
      if (w != std::nearbyint(w) || std::fabs(w) > 64.f) int_ok = false;
      bound += std::fabs((double)w) * 255.0 * (double)r[2] * (double)r[3] * (m.haar_tilted[(size_t)fi] ? 2.0 : 1.0);
    }
    if (bound >= 16777216.0) int_ok = false;
    SpecStump out;
    std::map<int, std::string> var;  // LDS offset -> variable holding that word
    auto var_of = [&](int ofs) {
      auto it = var.find(ofs);
      if (it != var.end()) return it->second;
      if (reuse) {
        auto r = reuse->find(ofs);
        if (r != reuse->end()) return var[ofs] = r->second;
      }
      snprintf(buf, sizeof(buf), "x%d_%d%s", local, (int)var.size(), win.c_str());
      const std::string name = buf;
      var[ofs] = name;
      out.decls += (out.decls.empty() ? "unsigned " : ", ") + name;
      snprintf(buf, sizeof(buf), "%s = (unsigned)%s[%d]; ", name.c_str(), tile_ptr.c_str(), ofs);
      out.loads += buf;
      return name;
    };
    std::string e = "{ float v = ";
    if (h16) {
      // 16-bit tile (TileGeom16). Range of the integer value V = sum_j w_j * S_j over all images: pixel p contributes
      // net(p) * I(p), I in [0, 255]. If [Vmin, Vmax] fits int16, V is the sign-extended low half of the same corner
      // combination computed with the 16-bit entries (the dropped high halves only add multiples of 2^16). Otherwise
      // every rectangle is summed exactly from strips whose sums fit 16 bits, and the strips' sums are combined in 32 bits.
      long long vmin = 0, vmax = 0;
      if (int_ok) {
        std::vector<int> net((size_t)(m.win_w + 1) * (size_t)(m.win_h + 1), 0);
        for (int j = 0; j < d.nrect; j++) {
          const int32_t* r = &m.haar_rects[(size_t)fi * 12 + j * 4];
          for (int yy = r[1]; yy < r[1] + r[3]; yy++)
            for (int xx = r[0]; xx < r[0] + r[2]; xx++) net[(size_t)yy * (size_t)(m.win_w + 1) + (size_t)xx] += (int)d.w[j];
        }
        for (int v : net) (v > 0 ? vmax : vmin) += 255LL * v;
      }
      if (int_ok && vmin >= -32768 && vmax <= 32767) {
        std::map<int, int> coef;  // 16-bit tile offset -> integer coefficient
        static const int sign[4] = {1, -1, -1, 1};
        for (int j = 0; j < d.nrect; j++) {
          const int32_t* r = &m.haar_rects[(size_t)fi * 12 + j * 4];
          const int o4[4] = {G16.at(r[1], r[0]), G16.at(r[1], r[0] + r[2]), G16.at(r[1] + r[3], r[0]), G16.at(r[1] + r[3], r[0] + r[2])};
          for (int k = 0; k < 4; k++) coef[o4[k]] += sign[k] * (int)d.w[j];
        }
        std::map<int, std::vector<int>> by_coef;
        for (auto& kv : coef)
          if (kv.second) by_coef[std::abs(kv.second)].push_back(kv.second > 0 ? kv.first + 1 : -(kv.first + 1));
        std::string tt;
        for (auto& g : by_coef) {
          std::string grp;
          for (int so : g.second) {
            grp += so > 0 ? (grp.empty() ? "" : " + ") : " - ";
            grp += var_of(std::abs(so) - 1);
          }
          if (grp.rfind(" - ", 0) == 0) grp = "0u" + grp;
          snprintf(buf, sizeof(buf), "%s%du * (", tt.empty() ? "" : " + ", g.first);
          tt += buf + grp + ")";
        }
        if (tt.empty()) tt = "0u";
        e += "(float)(int)(short)(" + tt + ")";
      } else {
        std::string terms_int, terms_float;
        for (int j = 0; j < d.nrect; j++) {
          const int32_t* r = &m.haar_rects[(size_t)fi * 12 + j * 4];
          std::string rj;
          for (const auto& pc : pieces16(r[0], r[1], r[2], r[3])) {
            const std::string a = var_of(G16.at(pc[1], pc[0])), b2 = var_of(G16.at(pc[1], pc[0] + pc[2])), c = var_of(G16.at(pc[1] + pc[3], pc[0])),
                              dd = var_of(G16.at(pc[1] + pc[3], pc[0] + pc[2]));
            rj += std::string(rj.empty() ? "" : " + ") + "((" + a + " - " + b2 + " - " + c + " + " + dd + ") & 0xffffu)";
          }
          if (rj.empty()) rj = "0u";
          snprintf(buf, sizeof(buf), "%s%d * (int)(", j ? " + " : "", (int)d.w[j]);
          terms_int += buf + rj + ")";
          terms_float += std::string(j ? " + " : "") + hexf(d.w[j]) + " * (float)(int)(" + rj + ")";
        }
        e += int_ok ? "(float)(" + terms_int + ")" : terms_float;
      }
    } else if (int_ok) {
      std::map<int, int> coef;  // LDS offset -> integer coefficient
      static const int sign[4] = {1, -1, -1, 1};
      for (int j = 0; j < d.nrect; j++)
        for (int k = 0; k < 4; k++) coef[d.ofs[j][k]] += sign[k] * (int)d.w[j];
      std::map<int, std::vector<int>> by_coef;  // |coefficient| -> signed offsets (+ofs+1 / -(ofs+1))
      for (auto& kv : coef)
        if (kv.second) by_coef[std::abs(kv.second)].push_back(kv.second > 0 ? kv.first + 1 : -(kv.first + 1));
      std::string tt;
      for (auto& g : by_coef) {
        std::string grp;
        for (int so : g.second) {
          grp += so > 0 ? (grp.empty() ? "" : " + ") : " - ";
          grp += var_of(std::abs(so) - 1);
        }
        if (grp.rfind(" - ", 0) == 0) grp = "0u" + grp;
        snprintf(buf, sizeof(buf), "%s%du * (", tt.empty() ? "" : " + ", g.first);  // unsigned: wrap-around is defined
        tt += buf + grp + ")";
      }
      if (tt.empty()) tt = "0u";
      e += "(float)(int)(" + tt + ")";
    } else {
      for (int j = 0; j < d.nrect; j++) {
        const std::string a = var_of(d.ofs[j][0]), b2 = var_of(d.ofs[j][1]), c = var_of(d.ofs[j][2]), dd = var_of(d.ofs[j][3]);
        e += std::string(j ? " + " : "") + hexf(d.w[j]) + " * (float)(int)(" + a + " - " + b2 + " - " + c + " + " + dd + ")";
      }
    }
    if (out.decls.empty()) out.decls = "";
    else out.decls += ";";
    // Sensitivity, measured on the headline bench with generated code that issued every LDS read twice (+68 % kernel time)
    // or did the value arithmetic twice (+1 %): the kernel is bound by the LDS pipeline, not by VALU issue.
    out.compute += e + vote_text(d, win, fixed_q, out);
    if (vars_out) *vars_out = var;
    return out;
  };
  // Corners shared between the stumps of a stage. A quarter of a late stage's corner reads fetch a word another stump of
  // the stage reads too (25x25 possible corners, 360-650 reads), but almost never the stump next to it. Where the stage sum
  // is exact (fixed-point votes: any order gives the same sum) the stumps are therefore re-ordered greedily -- next comes the
  // stump that shares most corners with the one before it -- and a stump takes those words from its predecessor's variables
  // instead of reading them again: 5-15 % fewer LDS reads in stages 1-7 of the bench cascade for one stump's worth of longer
  // live ranges. Not across the parts of a stage: a stump-split call starts at a part boundary with nothing loaded.
  const bool share_corners = !std::getenv("CCAMD_SPEC_NO_SHARE");
  int share_window = 1;  // a stump may take words from this many stumps before it
  if (const char* e = std::getenv("CCAMD_SPEC_SHARE_WINDOW")) share_window = std::max(1, std::min(8, std::atoi(e)));  // tuning
  auto corner_set = [&](const HaarStumpDev& d) {
    std::map<int, int> coef;
    static const int sign[4] = {1, -1, -1, 1};
    for (int j = 0; j < d.nrect; j++)
      for (int k = 0; k < 4; k++) coef[d.ofs[j][k]] += sign[k];
    std::vector<int> v;
    for (auto& kv : coef) v.push_back(kv.first);
    return v;
  };
  auto sharing_order = [&](int s, int step) {
    const int nt = m.stage_ntrees[(size_t)s], f0 = m.stage_first[(size_t)s];
    std::vector<std::vector<int>> pts((size_t)nt);
    for (int i = 0; i < nt; i++) pts[(size_t)i] = corner_set(t[step - 1][(size_t)f0 + i]);
    auto shared_with = [&](int i, const std::vector<int>& recent) {
      int n = 0;
      for (int o : pts[(size_t)i]) n += std::binary_search(recent.begin(), recent.end(), o) ? 1 : 0;
      return n;
    };
    auto part_start = [&](int n) {
      for (int k = 0; k < SPEC_PARTS; k++)
        if (n == (int)((long long)k * nt / SPEC_PARTS)) return true;
      return false;
    };
    std::vector<int> best_order;
    int best_total = -1;
    for (int start = 0; start < nt; start++) {  // greedy chain from every start; the one that saves most reads wins
      std::vector<int> order{start};
      std::vector<char> used((size_t)nt, 0);
      used[(size_t)start] = 1;
      int total = 0;
      for (int n = 1; n < nt; n++) {
        std::vector<int> recent;  // corners of the last `share_window` stumps
        for (int k = 1; k <= share_window && n - k >= 0; k++) {
          const std::vector<int>& q = pts[(size_t)order[(size_t)(n - k)]];
          recent.insert(recent.end(), q.begin(), q.end());
        }
        std::sort(recent.begin(), recent.end());
        int best = -1, best_shared = -1;
        for (int i = 0; i < nt; i++) {
          if (used[(size_t)i]) continue;
          const int sh = shared_with(i, recent);
          if (sh > best_shared) {
            best_shared = sh;
            best = i;
          }
        }
        used[(size_t)best] = 1;
        order.push_back(best);
        if (!part_start(n)) total += best_shared;  // nothing is carried across a part boundary
      }
      if (total > best_total) {
        best_total = total;
        best_order.swap(order);
      }
    }
    return best_order;
  };
  // Text that follows a stump's value expression "{ float v = ...": normalisation and the vote into the accumulator of
  // window `win` (closes the brace); records the constant part of a delta-form vote in `out`.
  vote_text = [&](const HaarStumpDev& d, const std::string& win, double fixed_q, SpecStump& out) -> std::string {
    if (delta_form && fixed_q > 0.) {
      char delta[64];
      const long long lq = (long long)std::llround((double)d.left / fixed_q), rq = (long long)std::llround((double)d.right / fixed_q);
      snprintf(delta, sizeof(delta), "0x%08x", (unsigned)(lq - rq));
      char vote[512];
      // The vote as TWO vector instructions: v_cmpx narrows EXEC to the lanes with v < thr (threshold as a 32-bit literal
      // operand), the delta is added under that mask (again a literal operand), and a scalar move puts EXEC back. A compare
      // and select costs four (move of the delta into a register, compare, select, add) plus a scalar move of the threshold.
      // `thr > v` is the comparison `v < thr` with the operands swapped: false for NaN either way. As asm the vote also keeps
      // the compiler from hoisting hundreds of constant deltas out of the stage loops and from re-associating the chain of
      // integer votes into a tree of partial sums, both of which it then has to spill.
      // (A three-instruction form without EXEC traffic -- compare into VCC, v_cndmask of a literal delta against a zero
      // register, add -- does not assemble: a VOP2 with a literal AND the implicit VCC read exceeds gfx9's constant bus.)
      unsigned thr_bits;
      std::memcpy(&thr_bits, &d.thr, 4);
      snprintf(vote, sizeof(vote),
               "; v *= vnf%s; { unsigned long long sx; asm volatile(\"s_mov_b64 %%1, exec\\n\\tv_cmpx_gt_f32_e32 0x%08x, %%2\\n\\tv_add_u32_e32 %%0, %s, %%0\\n\\ts_mov_b64 exec, %%1\" "
               ": \"+v\"(ai%s), \"=&s\"(sx) : \"v\"(v) : \"vcc\"); } }",
               win.c_str(), thr_bits, delta, win.c_str());
      out.base = (double)d.right;
      out.base_q = rq;
      return vote;
    }
    if (delta_form) {  // vote = right + (v < thr ? left - right : 0): the constant `right` is added once per part
      char delta[64];  // (hexf reuses `buf`)
      snprintf(delta, sizeof(delta), "%a", (double)d.left - (double)d.right);
      out.base = (double)d.right;
      return "; v *= vnf" + win + "; acc" + win + " += (v < " + hexf(d.thr) + " ? " + delta + " : 0.); }";
    }
    return "; v *= vnf" + win + "; acc" + win + " += (double)(v < " + hexf(d.thr) + " ? " + hexf(d.left) + " : " + hexf(d.right) + "); }";
  };
  for (int step = 1; step <= 2; step++) {
    snprintf(buf, sizeof(buf),
             "template <>\n__device__ %s double spec_stage<%d>(int st, int p_lo, int p_hi, const int32_t* b, float vnf) {\n", spec_stage_inline_attr(), step);
    o += buf;
    const bool h16 = tmode == TILE_16 && step == 2;  // STEP-2 tiles hold 16-bit entries
    if (h16) o += "  const unsigned short* h = reinterpret_cast<const unsigned short*>(b);\n";
    o += "  double acc = 0.;\n  switch (st) {\n";
    for (int s = 0; s < n_stages; s++) {
      snprintf(buf, sizeof(buf), "    case %d: {\n", s);
      o += buf;
      std::vector<SpecStump> st;
      double q = 0.;
      const bool fixed = delta_form && stage_quantum(m, s, q);
      if (fixed && share_corners) {
        const int nt = m.stage_ntrees[(size_t)s];
        const std::vector<int> order = sharing_order(s, step);
        std::vector<std::map<int, std::string>> hist;  // variable maps of the stumps of the current part, newest last
        for (int n = 0; n < nt; n++) {
          // spec_emit_stage cuts the stage into SPEC_PARTS contiguous parts at these positions
          for (int k = 0; k < SPEC_PARTS; k++)
            if (n == (int)((long long)k * nt / SPEC_PARTS)) hist.clear();
          std::map<int, std::string> recent, cur;
          for (int k = 0; k < share_window && k < (int)hist.size(); k++)
            for (auto& kv : hist[hist.size() - 1 - (size_t)k]) recent.insert(kv);
          const int i = order[(size_t)n];
          st.push_back(stump(t[step - 1][(size_t)m.stage_first[(size_t)s] + i], m.stage_first[(size_t)s] + i, i, "", q, h16, &recent, &cur));
          hist.push_back(cur);
        }
      } else
      for (int i = 0; i < m.stage_ntrees[(size_t)s]; i++)
        st.push_back(stump(t[step - 1][(size_t)m.stage_first[(size_t)s] + i], m.stage_first[(size_t)s] + i, i, "", fixed ? q : 0., h16));
      if (fixed) {
        o += "      unsigned ai = 0u;\n";
        spec_emit_stage(o, st, depth, true, {"ai"}, true);
        snprintf(buf, sizeof(buf), "      acc = (double)(int)ai * %a;\n", q);
        o += buf;
      } else
        spec_emit_stage(o, st, depth, true, {"acc"});
      o += "    } break;\n";
    }
    o += "    default: break;\n  }\n  return acc;\n}\n";
    // stage 0 for the two windows a thread owns in the dense phase: both windows' reads of a stump travel together
    snprintf(buf, sizeof(buf),
             "template <>\n__device__ __forceinline__ void spec_stage0_x2<%d>(const int32_t* ba, const int32_t* bb, float vnfa, float vnfb, double& "
             "acc_a, double& acc_b) {\n  double acca = 0., accb = 0.;\n  {\n",
             step);
    o += buf;
    if (h16)
      o += "  const unsigned short* ha = reinterpret_cast<const unsigned short*>(ba);\n  const unsigned short* hb = reinterpret_cast<const unsigned short*>(bb);\n";
    {
      std::vector<SpecStump> st;
      double q = 0.;
      const bool fixed = delta_form && stage_quantum(m, 0, q);
      for (int i = 0; i < m.stage_ntrees[0]; i++) {
        const HaarStumpDev& d = t[step - 1][(size_t)m.stage_first[0] + i];
        SpecStump a = stump(d, m.stage_first[0] + i, i, "a", fixed ? q : 0., h16), b2 = stump(d, m.stage_first[0] + i, i, "b", fixed ? q : 0., h16);
        st.push_back(SpecStump{a.loads + b2.loads, a.decls + " " + b2.decls, a.compute + " " + b2.compute, a.base, a.base_q});
      }
      if (fixed) {
        o += "      unsigned aia = 0u, aib = 0u;\n";
        spec_emit_stage(o, st, depth, false, {"aia", "aib"}, true);
        snprintf(buf, sizeof(buf), "      acca = (double)(int)aia * %a;\n      accb = (double)(int)aib * %a;\n", q, q);
        o += buf;
      } else
        spec_emit_stage(o, st, depth, false, {"acca", "accb"});
    }
    o += "  }\n  acc_a = acca;\n  acc_b = accb;\n}\n";
  }
  return o;
}

// LBP variant: the 16 lattice offsets are immediates; the 256-bit subsets stay a (module-resident) table because the word
// a lane needs depends on its own code. Integer arithmetic throughout, the expression of stump_vote().
static std::string spec_stage_source_lbp(const Cascade& m, int n_stages, bool tile16) {
  std::vector<LbpStumpDev> t[2];
  build_lbp_stumps<1>(m, t[0]);
  if (tile16)
    build_lbp_stumps16(m, t[1]);
  else
    build_lbp_stumps<2>(m, t[1]);
  n_stages = std::min<int>(n_stages, (int)m.stage_ntrees.size());
  const int depth = 0;  // 16 independent words per stump already: no explicit pipelining measured best (7.8 ms per 32 frames; one stump ahead 8.2, two 8.9)
  std::string o;
  char buf[1024];
  auto hexf = [&](float v) {
    char b2[64];
    snprintf(b2, sizeof(b2), "%af", (double)v);
    return std::string(b2);
  };
  auto stump = [&](const LbpStumpDev& d, int local, const std::string& win, bool h16) {
    SpecStump out;
    std::string P[16];
    for (int k = 0; k < 16; k++) {
      snprintf(buf, sizeof(buf), "p%d_%d%s", local, k, win.c_str());
      P[k] = buf;
      out.decls += (k ? ", " : "int ") + P[k];
      snprintf(buf, sizeof(buf), "%s = %s%s[%d]; ", P[k].c_str(), h16 ? "h" : "b", win.c_str(), d.ofs[k]);
      out.loads += buf;
    }
    out.decls += ";";
    // 16-bit tile: a cell sum is the low half of the corner combination (exact: 255 * cell area < 2^16, tile16_eligible)
    // Cells from horizontal differences: the 12 differences of neighbouring lattice points of a row, then one subtraction
    // per cell (21 integer operations instead of 27).
    std::string diffs = "const int ";
    bool firstd = true;
    for (int k = 0; k < 15; k++) {
      if (k % 4 == 3) continue;
      snprintf(buf, sizeof(buf), "%sh%d_%d%s = %s - %s", firstd ? "" : ", ", local, k, win.c_str(), P[k].c_str(), P[k + 1].c_str());
      diffs += buf;
      firstd = false;
    }
    diffs += "; ";
    // the cell with corners a, a + 1 (top) and c, c + 1 (bottom): h_a - h_c
    auto cell = [&](int a, int /*a + 1*/, int c, int /*c + 1*/) {
      char hb[96];
      snprintf(hb, sizeof(hb), "h%d_%d%s - h%d_%d%s", local, a, win.c_str(), local, c, win.c_str());
      const std::string v = hb;
      return h16 ? "((" + v + ") & 0xffff)" : v;
    };
    // The 256-bit subset as eight literals picked by the three top bits of the code -- the results of the first three
    // comparisons -- through seven unconditional selects, instead of a load from a table: the table word depends on the
    // lane's own code, so it is a vector memory load whose latency sits in every stump's dependency chain, and the late
    // stages (a handful of windows per tile) are nothing but that chain.
    const int* w = d.subset;
    std::string t = "{ " + diffs + "const int c = " + cell(5, 6, 9, 10) + "; const bool b7 = " + cell(0, 1, 4, 5) + " >= c, b6 = " + cell(1, 2, 5, 6) +
                    " >= c, b5 = " + cell(2, 3, 6, 7) + " >= c; const int lo = (" + cell(6, 7, 10, 11) + " >= c ? 16 : 0) | (" +
                    cell(10, 11, 14, 15) + " >= c ? 8 : 0) | (" + cell(9, 10, 13, 14) + " >= c ? 4 : 0) | (" + cell(8, 9, 12, 13) +
                    " >= c ? 2 : 0) | (" + cell(4, 5, 8, 9) + " >= c ? 1 : 0); ";
    snprintf(buf, sizeof(buf),
             "const unsigned l0 = b5 ? 0x%08xu : 0x%08xu, l1 = b5 ? 0x%08xu : 0x%08xu, l2 = b5 ? 0x%08xu : 0x%08xu, l3 = b5 ? 0x%08xu : 0x%08xu; "
             "const unsigned m0 = b6 ? l1 : l0, m1 = b6 ? l3 : l2; const unsigned sw = b7 ? m1 : m0; "
             "acc%s += (double)(((sw >> lo) & 1u) ? %s : %s); }",
             (unsigned)w[1], (unsigned)w[0], (unsigned)w[3], (unsigned)w[2], (unsigned)w[5], (unsigned)w[4], (unsigned)w[7], (unsigned)w[6],
             win.c_str(), hexf(d.left).c_str(), hexf(d.right).c_str());
    out.compute = t + buf;
    return out;
  };
  for (int step = 1; step <= 2; step++) {
    snprintf(buf, sizeof(buf),
             "template <>\n__device__ %s double spec_stage<%d>(int st, int p_lo, int p_hi, const int32_t* b, float vnf) {\n", spec_stage_inline_attr(), step);
    o += buf;
    const bool h16 = tile16 && step == 2;  // STEP-2 tiles hold 16-bit entries
    if (h16) o += "  const unsigned short* h = reinterpret_cast<const unsigned short*>(b);\n";
    o += "  double acc = 0.;\n  switch (st) {\n";
    for (int s = 0; s < n_stages; s++) {
      snprintf(buf, sizeof(buf), "    case %d: {\n", s);
      o += buf;
      std::vector<SpecStump> st;
      for (int i = 0; i < m.stage_ntrees[(size_t)s]; i++) {
        const int idx = m.stage_first[(size_t)s] + i;
        st.push_back(stump(t[step - 1][(size_t)idx], i, "", h16));
      }
      spec_emit_stage(o, st, depth, true, {"acc"});
      o += "    } break;\n";
    }
    o += "    default: break;\n  }\n  return acc;\n}\n";
    snprintf(buf, sizeof(buf),
             "template <>\n__device__ __forceinline__ void spec_stage0_x2<%d>(const int32_t* ba, const int32_t* bb, float vnfa, float vnfb, double& "
             "acc_a, double& acc_b) {\n  double acca = 0., accb = 0.;\n  {\n",
             step);
    o += buf;
    if (h16)
      o += "  const unsigned short* ha = reinterpret_cast<const unsigned short*>(ba);\n  const unsigned short* hb = reinterpret_cast<const unsigned short*>(bb);\n";
    {
      std::vector<SpecStump> st;
      for (int i = 0; i < m.stage_ntrees[0]; i++) {
        const int idx = m.stage_first[0] + i;
        SpecStump a = stump(t[step - 1][(size_t)idx], i, "a", h16), b2 = stump(t[step - 1][(size_t)idx], i, "b", h16);
        st.push_back(SpecStump{a.loads + b2.loads, a.decls + " " + b2.decls, a.compute + " " + b2.compute});
      }
      spec_emit_stage(o, st, depth, false, {"acca", "accb"});
    }
    o += "  }\n  acc_a = acca;\n  acc_b = accb;\n}\n";
  }
  return o;
}

// ------------------------------------------------------------------------------------------------
// Compilation with hiprtc (loaded on demand: the library does not link against it) and the code-object caches.
// ------------------------------------------------------------------------------------------------
struct HipRtcApi {
  void* lib = nullptr;
  int (*create)(void**, const char*, const char*, int, const char* const*, const char* const*) = nullptr;
  int (*compile)(void*, int, const char* const*) = nullptr;
  int (*log_size)(void*, size_t*) = nullptr;
  int (*log)(void*, char*) = nullptr;
  int (*code_size)(void*, size_t*) = nullptr;
  int (*code)(void*, char*) = nullptr;
  int (*destroy)(void**) = nullptr;
  int (*version)(int*, int*) = nullptr;  // optional
  bool ok() const { return create && compile && log_size && log && code_size && code && destroy; }
};

static const HipRtcApi& hiprtc_api() {
  static HipRtcApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char* name : {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (api.lib) break;
    }
    if (!api.lib) return;
    auto sym = [&](const char* n) { return dlsym(api.lib, n); };
    api.create = reinterpret_cast<decltype(api.create)>(sym("hiprtcCreateProgram"));
    api.compile = reinterpret_cast<decltype(api.compile)>(sym("hiprtcCompileProgram"));
    api.log_size = reinterpret_cast<decltype(api.log_size)>(sym("hiprtcGetProgramLogSize"));
    api.log = reinterpret_cast<decltype(api.log)>(sym("hiprtcGetProgramLog"));
    api.code_size = reinterpret_cast<decltype(api.code_size)>(sym("hiprtcGetCodeSize"));
    api.code = reinterpret_cast<decltype(api.code)>(sym("hiprtcGetCode"));
    api.destroy = reinterpret_cast<decltype(api.destroy)>(sym("hiprtcDestroyProgram"));
    api.version = reinterpret_cast<decltype(api.version)>(sym("hiprtcVersion"));
  });
  return api;
}

// hiprtc has no <cstdint>: the fixed-width names the kernel source uses
static const char kSpecPrelude[] =
    "typedef signed char int8_t;\ntypedef unsigned char uint8_t;\ntypedef short int16_t;\ntypedef unsigned short uint16_t;\n"
    "typedef int int32_t;\ntypedef unsigned int uint32_t;\ntypedef long long int64_t;\ntypedef unsigned long long uint64_t;\n";

// Compiles `src` for `arch`; identical (source, options) pairs are served from a per-process cache.
// The modules a run-time specialised kernel is compiled as: which tiles each covers and its tile height (-DCC_TILE_Y).
// * LBP kernels whose STEP-2 tiles hold 16-bit entries: ONE module, 20 window rows per tile (64 x 20 windows per block of 256
//   threads). A tile's halo rows are staged per 20 instead of per 8 window rows, the per-block work (barrier rounds,
//   counters, the wave phase's window collection) is paid once per 1 280 windows, and the late stages find 2.5 x the windows per
//   block to fill their wavefronts with; at 26 KB per block six blocks fit a CU (6 wavefronts per SIMD: 80 VGPRs).
//   Stock LBP cascade, ms per 32 Full-HD frames alone (round-4 run, script not kept): 8 rows 4.90, 12 rows 4.25, 16 rows 3.96, 20 rows 3.78,
//   24 rows 3.85, 32 rows 4.12 (each at its best register budget).
// * Haar kernels with 32-bit tiles: TWO modules, one per step -- 20 rows for the STEP-1 tiles, 10 for the STEP-2 tiles
//   (spec_step2_rows; 8 in the padded layout until profiles/EXPERIMENTS.md 3.24). A
//   STEP-1 tile is a third of a STEP-2 tile (12.7 KB against 24 KB at 12 rows), but one launch requests the larger of the two
//   for every block. ms per 32 Full-HD frames alone, one run (round-4 run, script not kept): one module at 8 rows 8.35; two
//   modules at 8 / 8 rows 7.82, 12 / 8 rows 7.32, 12 / 12 rows 7.49, 16 / 12 rows 7.77, 12 / 16 rows 8.11 (STEP-1 / STEP-2; a
//   32-bit STEP-2 tile of 12 rows leaves 4 blocks per CU). The STEP-1 module has the lean LDS layout (eval_lds_bytes), a
//   register budget for the blocks its own request allows, and a wave_below of its own (spec_wave_below); for a 24x24 window
//   12 / 16 / 20 / 24 rows are 19.2 / 22.7 / 26.1 / 29.6 KB per block = 8 / 7 / 6 / 5 blocks per CU, and its launch takes
//   2.61 / 2.97 / 2.45 / 2.77 ms per 32 frames (2.78 / 2.99 / 2.65 / 3.09 with the padded layout at 7 / 6 / 5 / 4 blocks;
//   profiles/EXPERIMENTS.md 3.22). Larger windows: spec_step1_rows. The STEP-2 module has the same layout and the detector's
//   wave_below; its launch takes 4.24 ms at 8 rows padded, 4.33 / 4.20 / 4.05 / 4.48 / 4.33 ms at 8 / 9 / 10 / 11 / 12 rows lean.
// * everything else (Haar with 16-bit tiles): one module at the library's 8 rows.
// CCAMD_SPEC_TILE_Y sets every module's rows, CCAMD_SPEC_TILE_Y1 / _Y2 the STEP-1 / STEP-2 module's (the Haar STEP-2 module: any
// height from 8 to 12), CCAMD_SPEC_ONE_MODULE=1
// forces a single module (tuning).
struct SpecModulePlan {
  int only_step, tile_y;
};
// The Haar modules of one step each take the lean LDS layout (eval_lds_bytes; compiled with CC_LEAN_LDS): their tiles grow
// taller than the library's. (Tilted cascades never get a module per step.)
static bool spec_lean_lds(const Cascade& m, int tmode, int only_step) {
  return (only_step == 1 || only_step == 2) && tmode == TILE_32 && m.feature_type == CC_FEATURE_HAAR && !m.has_tilted;
}
// LDS request of one block of the STEP-1 / STEP-2 Haar module at `tile_y` window rows (lean layout).
static size_t spec_step1_lds(const Cascade& m, int tile_y) {
  return eval_lds_bytes(TileGeom<1>(m.win_w, m.win_h, tile_y).words(), false, true, tile_y, true);
}
static size_t spec_step2_lds(const Cascade& m, int tile_y) {
  return eval_lds_bytes(TileGeom<2>(m.win_w, m.win_h, tile_y).words(), false, true, tile_y, true);
}
static size_t spec_lean_request(const Cascade& m, int only_step, int tile_y) {
  return only_step == 2 ? spec_step2_lds(m, tile_y) : spec_step1_lds(m, tile_y);
}
// Window rows of the STEP-1 Haar module's tiles: `want`, or for windows whose tile is too large for that, the tallest
// height below it (a multiple of the block's wavefronts) that still lets kSpecStep1MinBlocks blocks share a CU -- below that
// the late stages of one block are no longer hidden by the others. Never less than the library's TILE_Y: a window that large
// (128x40, 96x96) fits fewer blocks at any height.
constexpr int kSpecStep1Rows = 20;
constexpr int kSpecStep1MinBlocks = 4;
static int spec_step1_rows(const Cascade& m, int want) {
  int ty = want;
  while (ty - EVAL_WAVES >= TILE_Y && lds_blocks_per_cu(spec_step1_lds(m, ty)) < kSpecStep1MinBlocks) ty -= EVAL_WAVES;
  return ty;
}
// Window rows of the STEP-2 Haar module's tiles: the tallest height from the library's TILE_Y up to kSpecStep2MaxRows whose
// lean request runs as many blocks on a CU as the lean request at TILE_Y rows does, counted in allocation units
// (lds_blocks_resident). 24x24: 10 rows, 32 000 bytes = 25 units, 5 blocks like the 8 rows before them; 11 rows are 27 units
// and 4 blocks. A taller tile pools more windows per block -- fuller table rows in the compacted stages, the per-block work
// of every stage paid once per more windows -- and a STEP-2 tile that costs a resident block for it has never paid
// (profiles/EXPERIMENTS.md 3.2, 3.24). The lean request at TILE_Y rows is below the padded one of the module it replaces, so
// no window size ends with fewer blocks than it had. Any height is allowed: see WIN_PER_THREAD for heights that are no
// multiple of the block's wavefronts.
constexpr int kSpecStep2MaxRows = 12;
static int spec_step2_rows(const Cascade& m) {
  const int blocks = lds_blocks_resident(spec_step2_lds(m, TILE_Y));
  if (blocks < 1) return TILE_Y;  // a window whose 8-row tile exceeds the CU's LDS: no height helps
  int ty = TILE_Y;
  while (ty + 1 <= kSpecStep2MaxRows && lds_blocks_resident(spec_step2_lds(m, ty + 1)) >= blocks) ty++;
  return ty;
}
// Blocks per CU a lean module's register budget is compiled for.
static int spec_lean_blocks(const Cascade& m, int only_step, int tile_y) {
  return only_step == 2 ? lds_blocks_resident(spec_step2_lds(m, tile_y)) : lds_blocks_per_cu(spec_step1_lds(m, tile_y));
}
// EvalArgs::wave_below of one module. The detector's value (configure_detector: 24) was tuned on tiles of 8 window rows. The
// module of STEP-1 tiles pools 768 and more windows per block, and its blocks reach the wave phase with more windows each:
// kStep1WaveBelow for tiles of 12 rows and more (measured at 12 and 20 rows: 16 +4.9 / +3.2 %, 24 0, 32 -1.2 / -1.8 %, 40 and
// 56 at 20 rows -0.4 / -0.5 %; profiles/EXPERIMENTS.md 3.22). -1 = the detector's value: every other module, a wave phase
// that is off, and under CCAMD_WAVE_BELOW (which then holds for all modules). CCAMD_WAVE_BELOW1 / CCAMD_WAVE_BELOW2: the STEP-1 /
// STEP-2 module's value (tuning).
constexpr int kStep1WaveBelow = 32;
int spec_wave_below(int detector_value, int only_step, int tile_y) {
  if ((only_step != 1 && only_step != 2) || detector_value <= 0) return -1;
  if (const char* e = std::getenv(only_step == 1 ? "CCAMD_WAVE_BELOW1" : "CCAMD_WAVE_BELOW2")) return std::max(0, std::min(64, std::atoi(e)));
  // the STEP-2 module keeps the detector's value: at 10 rows 32 and 40 are within the spread of 24 (profiles/EXPERIMENTS.md 3.24)
  if (only_step == 2) return -1;
  if (std::getenv("CCAMD_WAVE_BELOW") || tile_y < 12) return -1;
  return std::max(detector_value, kStep1WaveBelow);
}

static std::vector<SpecModulePlan> spec_modules(const Cascade& m, int tmode) {
  // the STEP-2 Haar module takes any height from the library's to kSpecStep2MaxRows, every other module whole rows per wavefront
  auto valid = [&](int ty, bool any_height) {
    return any_height ? ty >= TILE_Y && ty <= kSpecStep2MaxRows : ty >= EVAL_WAVES && ty <= 32 && ty % EVAL_WAVES == 0;
  };
  auto env_rows = [&](const char* name, int dflt, bool any_height = false) {
    const char* e = std::getenv(name);
    const int v = e ? std::atoi(e) : dflt;
    return valid(v, any_height) ? v : dflt;
  };
  // (cascades with tilted features keep the library's tile height: their records and generated offsets carry the distance
  // between the sum tile and the tilted tile behind it, which depends on the tile's rows)
  if (m.has_tilted) return {{0, TILE_Y}};
  const bool lbp16 = m.feature_type == CC_FEATURE_LBP && tmode == TILE_16;
  const bool haar32 = tmode == TILE_32 && m.feature_type == CC_FEATURE_HAAR;
  const bool rows_given = std::getenv("CCAMD_SPEC_TILE_Y") != nullptr;
  const int all = env_rows("CCAMD_SPEC_TILE_Y", lbp16 ? 20 : TILE_Y);
  const bool two = (haar32 || std::getenv("CCAMD_SPEC_TWO_MODULES")) && !std::getenv("CCAMD_SPEC_ONE_MODULE");
  if (!two) return {{0, all}};
  const bool lean2 = spec_lean_lds(m, tmode, 2);
  return {{2, env_rows("CCAMD_SPEC_TILE_Y2", (lean2 && !rows_given) ? spec_step2_rows(m) : all, lean2)}, {1, env_rows("CCAMD_SPEC_TILE_Y1", (haar32 && !rows_given) ? spec_step1_rows(m, kSpecStep1Rows) : all)}};
}

// lean_blocks: 0, or this is the module with the lean LDS layout and its LDS request lets that many blocks share a CU.
static cc_status compile_specialised(const std::string& src, const std::string& arch, int n_stages, bool lbp, int tmode, int tile_y, int only_step, int win_w, int win_h,
                                     int lean_blocks, std::vector<char>& code) {
  const bool tile16 = tmode == TILE_16;
  static std::mutex mu;
  static std::map<std::string, std::vector<char>> cache;
  const std::string o_arch = "--offload-arch=" + arch, o_k = "-DCC_SPEC_STAGES=" + std::to_string(n_stages);
  const std::string o_ty = "-DCC_TILE_Y=" + std::to_string(tile_y), o_th = "-DCC_EVAL_THREADS=" + std::to_string(EVAL_THREADS);
  // same code generation rules as the ahead-of-time build (Makefile): no FMA contraction, no fast-math
  // register budget = the occupancy the LDS footprint allows: 5 blocks per CU with the 32-bit tile, 7-8 with the 16-bit one
  // (16-bit tiles of >= 20 rows: 26 KB per block = 6 blocks per CU)
  // (lean module: what its own request allows, a block being one wavefront per SIMD; CCAMD_SPEC_WAVES1 overrides, tuning)
  int min_waves = tile16 ? (tile_y >= 20 ? 6 : 7) : CC_EVAL_MIN_WAVES_PER_EU;
  if (lean_blocks > 0) {
    min_waves = std::max(1, std::min(8, lean_blocks * EVAL_WAVES / 4));
    if (const char* e = only_step == 1 ? std::getenv("CCAMD_SPEC_WAVES1") : nullptr) min_waves = std::max(1, std::min(8, std::atoi(e)));
  }
  const std::string o_w = "-DCC_EVAL_MIN_WAVES_PER_EU=" + std::to_string(min_waves);
  const std::string o_step = "-DCC_ONLY_STEP=" + std::to_string(only_step);
  const std::string o_w0 = "-DCC_SPEC_W0=" + std::to_string(win_w), o_h0 = "-DCC_SPEC_H0=" + std::to_string(win_h);  // tile geometry folds to constants
  std::vector<const char*> optv = {o_arch.c_str(), "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", o_k.c_str(), o_ty.c_str(), o_th.c_str(), o_w.c_str(), o_w0.c_str(), o_h0.c_str()};
  if (only_step) optv.push_back(o_step.c_str());
  if (lbp) optv.push_back("-DCC_SPEC_LBP");
  if (tile16) optv.push_back("-DCC_SPEC_TILE16");
  if (lean_blocks > 0) optv.push_back("-DCC_LEAN_LDS");
  const char* const* opts = optv.data();
  const int n_opts = (int)optv.size();
  std::string key;  // everything the code object depends on: compiler version, options, then the source
  {
    int major = 0, minor = 0;
    const HipRtcApi& rtc = hiprtc_api();
    if (rtc.version) (void)rtc.version(&major, &minor);
    key += "hiprtc " + std::to_string(major) + "." + std::to_string(minor) + " ";
  }
  for (int i = 0; i < n_opts; i++) key += std::string(opts[i]) + " ";
  key += "#" + src;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) {
      code = it->second;
      return CC_OK;
    }
  }
  // second level: code objects on disk ($CCAMD_CACHE_DIR, else ~/.cache/cascadeclassifier_amd; CCAMD_CACHE_DIR= disables).
  // The file is named by a 64-bit FNV-1a hash of the key and starts with a header that repeats the key's length and two
  // independent 64-bit hashes of it; the key covers architecture, options, the hiprtc version and the generated source.
  // A file whose header does not match (another toolchain, a collision, a foreign or truncated file) is ignored and
  // rewritten: a wrong code object would carry another cascade's thresholds and give wrong detections silently.
  struct CacheHeader {
    char magic[8];
    unsigned long long key_len, h1, h2;
  };
  auto hash_key = [&](unsigned long long seed, unsigned long long prime) {
    unsigned long long h = seed;
    for (unsigned char ch : key) h = (h ^ ch) * prime;
    return h ^ (h >> 29);
  };
  CacheHeader want;
  std::memcpy(want.magic, "CCAMDSP2", 8);
  want.key_len = key.size();
  want.h1 = hash_key(1469598103934665603ull, 1099511628211ull);
  want.h2 = hash_key(0x9E3779B97F4A7C15ull, 0x100000001B3ull * 31ull + 2ull);
  std::string cache_file;
  {
    const char* dir = std::getenv("CCAMD_CACHE_DIR");
    std::string base;
    if (dir)
      base = dir;
    else if (const char* home = std::getenv("HOME"))
      base = std::string(home) + "/.cache/cascadeclassifier_amd";
    if (!base.empty()) {
      char name[64];
      snprintf(name, sizeof(name), "/spec_%016llx_%zu.hsaco", want.h1, key.size());
      cache_file = base + name;
      if (FILE* f = std::fopen(cache_file.c_str(), "rb")) {
        std::fseek(f, 0, SEEK_END);
        const long n = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        CacheHeader got;
        std::vector<char> buf;
        bool ok = n > (long)sizeof(CacheHeader) + 64 && std::fread(&got, sizeof(got), 1, f) == 1 && std::memcmp(&got, &want, sizeof(want)) == 0;
        if (ok) {
          buf.resize((size_t)n - sizeof(CacheHeader));
          ok = std::fread(buf.data(), 1, buf.size(), f) == buf.size() && std::memcmp(buf.data(), "\x7f" "ELF", 4) == 0;
        }
        std::fclose(f);
        if (ok) {
          code = buf;
          std::lock_guard<std::mutex> lk(mu);
          cache[key] = code;
          return CC_OK;
        }
      }
      (void)::mkdir(base.c_str(), 0755);  // one level; a missing parent just means no disk cache
    }
  }
  if (const char* dump = std::getenv("CCAMD_DUMP_SPEC_SOURCE")) {  // for inspection with hipcc -S
    if (FILE* f = std::fopen(dump, "w")) {
      std::fwrite(src.data(), 1, src.size(), f);
      std::fclose(f);
    }
  }
  // One compilation at a time per process: builds are rare and seconds long, the compiler stack underneath hiprtc is not
  // worth trusting with concurrent invocations, and a second thread asking for the same code waits here and then finds it.
  static std::mutex compile_mu;
  std::lock_guard<std::mutex> compile_lock(compile_mu);
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) {
      code = it->second;
      return CC_OK;
    }
  }
  const HipRtcApi& rtc = hiprtc_api();
  if (!rtc.ok()) return set_error(CC_ERR_UNSUPPORTED, "cc_detector_specialize: libhiprtc is not available (%s)", rtc.lib ? "missing symbols" : "dlopen failed");
  void* prog = nullptr;
  if (rtc.create(&prog, src.c_str(), "cc_eval_kernel_spec.hip", 0, nullptr, nullptr) != 0)
    return set_error(CC_ERR_HIP, "cc_detector_specialize: hiprtcCreateProgram failed");
  const int rc = rtc.compile(prog, n_opts, const_cast<const char**>(opts));
  if (rc != 0) {
    size_t n = 0;
    rtc.log_size(prog, &n);
    std::string log(n + 1, '\0');
    if (n) rtc.log(prog, &log[0]);
    rtc.destroy(&prog);
    return set_error(CC_ERR_HIP, "cc_detector_specialize: hiprtc compilation failed (%d): %.1500s", rc, log.c_str());
  }
  size_t n = 0;
  rtc.code_size(prog, &n);
  code.resize(n);
  rtc.code(prog, code.data());
  rtc.destroy(&prog);
  if (!cache_file.empty()) {  // write to a private name, then rename: readers never see a partial file
    const std::string tmp = cache_file + "." + std::to_string((long long)::getpid()) + ".tmp";
    if (FILE* f = std::fopen(tmp.c_str(), "wb")) {
      const bool ok = std::fwrite(&want, sizeof(want), 1, f) == 1 && std::fwrite(code.data(), 1, code.size(), f) == code.size();
      std::fclose(f);
      if (!ok || std::rename(tmp.c_str(), cache_file.c_str()) != 0) (void)std::remove(tmp.c_str());
    }
  }
  std::lock_guard<std::mutex> lk(mu);
  cache[key] = code;
  return CC_OK;
}

// Host half of the specialisation: source for the first stages (whole stages within the code-size budget) compiled for
// `arch`. No device calls: safe on a background thread.
cc_status spec_build(const Cascade& m, int n_stages, const std::string& arch, std::vector<SpecCode>& codes, int& k_out, int& tmode_out) {
  if (cc_status hs = refuse_hog(m, "cc_detector_specialize"); hs != CC_OK) return hs;
  if (m.max_nodes_per_tree > 1) return set_error(CC_ERR_UNSUPPORTED, "cc_detector_specialize: stump cascades only");
  int k = 0, stumps = 0;
  const int budget = 320;  // instruction cache: more stages measured no faster, 12 stages slower
  while (k < (int)m.stage_ntrees.size() && k < n_stages && k < MAX_STAGES && (k == 0 || stumps + m.stage_ntrees[(size_t)k] <= budget))
    stumps += m.stage_ntrees[(size_t)k++];
  std::string src = kSpecPrelude;
  src += "namespace ccamd {\n";
  src += kEvalKernelSrc;
  src += "\n}  // namespace ccamd\n";
  const std::string marker = "//@@CC_SPEC_FUNCTIONS@@";
  const size_t pos = src.find(marker);
  if (pos == std::string::npos) return set_error(CC_ERR_HIP, "cc_detector_specialize: kernel source has no specialisation marker");
  const int tmode = tile16_eligible(m, k) ? TILE_16 : TILE_32;
  src.replace(pos, marker.size(), spec_stage_source(m, k, tmode));
  k_out = k;
  tmode_out = tmode;
  codes.clear();
  for (const SpecModulePlan& mp : spec_modules(m, tmode)) {
    SpecCode c;
    c.only_step = mp.only_step;
    c.tile_y = mp.tile_y;
    const int lean_blocks = spec_lean_lds(m, tmode, mp.only_step) ? std::max(1, spec_lean_blocks(m, mp.only_step, mp.tile_y)) : 0;
    const cc_status st = compile_specialised(src, arch, k, m.feature_type == CC_FEATURE_LBP, tmode, mp.tile_y, mp.only_step, m.win_w, m.win_h, lean_blocks, c.code);
    if (st != CC_OK) return st;
    codes.push_back(std::move(c));
  }
  return CC_OK;
}

// Device half of the specialisation: loads the code objects of spec_build and sizes each module's LDS request from the
// tiles it stages (`base_lds`: what the ahead-of-time kernels request). out[0] is the module for all tiles or for the STEP-2
// tiles, out[1] the STEP-1 module if there is one. On failure nothing stays loaded.
cc_status spec_load(const Cascade& m, const std::vector<SpecCode>& codes, int tmode, size_t base_lds, SpecModule out[2], int* n_out) {
  if (codes.empty() || codes.size() > 2) return set_error(CC_ERR_HIP, "cc_detector_specialize: %zu modules", codes.size());
  const bool haar_k = m.feature_type == CC_FEATURE_HAAR;
  int n = 0;
  auto fail = [&](SpecModule& x) {
    (void)hipGetLastError();
    if (x.mod) (void)hipModuleUnload(x.mod);
    for (int i = 0; i < n; i++) (void)hipModuleUnload(out[i].mod);
  };
  for (const SpecCode& c : codes) {
    SpecModule x;
    x.tile_y = c.tile_y;
    x.only_step = c.only_step;  // tiles this module stages: of the step(s) it covers
    const char* entry = c.only_step == 1 ? "k_eval_spec_step1" : c.only_step == 2 ? "k_eval_spec_step2" : "k_eval_spec";
    if (hipModuleLoadData(&x.mod, c.code.data()) != hipSuccess || hipModuleGetFunction(&x.fn, x.mod, entry) != hipSuccess) {
      fail(x);
      return set_error(CC_ERR_HIP, "cc_detector_specialize: the compiled module does not load or has no entry point");
    }
    const int ty = c.tile_y, step = c.only_step;
    x.lds = base_lds;
    if (tmode == TILE_32) {
      const TileGeom<1> G1(m.win_w, m.win_h, ty);
      const TileGeom<2> G2(m.win_w, m.win_h, ty);
      const int words = step == 1 ? G1.words() : step == 2 ? G2.words() : std::max(G1.words(), G2.words());
      x.lds = spec_lean_lds(m, tmode, step) ? spec_lean_request(m, step, ty) : eval_lds_bytes(words, m.has_tilted, haar_k, ty);
    } else if (tmode == TILE_16) {  // STEP-1 tile in 32 bits, STEP-2 tile in 16 bits
      const TileGeom<1> G1(m.win_w, m.win_h, ty);
      const TileGeom16 G2(m.win_w, m.win_h, ty);
      x.lds = eval_lds_bytes(std::max(G1.words(), G2.words()), false, haar_k, ty);
    }
    if (x.lds > 64 * 1024) {  // same opt-in as the ahead-of-time kernels (cc_detector_create)
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(x.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x.lds);
      if (e != hipSuccess) {
        fail(x);
        return set_error(CC_ERR_UNSUPPORTED, "cc_detector_specialize: %zu bytes of LDS per tile cannot be requested for a run-time module (%s)",
                         x.lds, hipGetErrorString(e));
      }
    }
    if (std::getenv("CCAMD_TRACE_HOST")) {  // what the specialised kernel's footprint allows per CU
      int nb = 0, scratch = -1;
      if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, x.fn, EVAL_THREADS, x.lds) != hipSuccess) (void)hipGetLastError();
      if (hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, x.fn) != hipSuccess) (void)hipGetLastError();
      std::fprintf(stderr, "[ccamd host] specialised kernel: tile mode %d, tiles of step %d (0 = all), %d window rows, %zu bytes of LDS per block, %d resident blocks per CU, %d bytes of scratch per lane\n",
                   tmode, c.only_step, ty, x.lds, nb, scratch);
    }
    out[n++] = x;
  }
  if (n == 2 && out[0].only_step == 1) std::swap(out[0], out[1]);
  *n_out = n;
  return CC_OK;
}

}  // namespace ccamd

using namespace ccamd;

extern "C" {

cc_status cc_debug_spec_step1_plan(const cc_cascade* c, int rows_wanted, int wave_below_detector, int* rows, size_t* lds_bytes, int* blocks_per_cu,
                                   int* wave_below) {
  if (!c) return set_error(CC_ERR_INVALID_ARG, "cc_debug_spec_step1_plan: null cascade");
  if (cc_status hs = refuse_hog(c->m, "cc_debug_spec_step1_plan"); hs != CC_OK) return hs;
  if (c->m.max_nodes_per_tree > 1 || !spec_lean_lds(c->m, TILE_32, 1))
    return set_error(CC_ERR_UNSUPPORTED, "cc_debug_spec_step1_plan: upright Haar stump cascades only");
  const int ty = rows_wanted > 0 ? rows_wanted : spec_step1_rows(c->m, kSpecStep1Rows);
  if (ty < EVAL_WAVES || ty > 32 || ty % EVAL_WAVES) return set_error(CC_ERR_INVALID_ARG, "cc_debug_spec_step1_plan: %d window rows per tile", ty);
  const size_t lds = spec_step1_lds(c->m, ty);
  if (rows) *rows = ty;
  if (lds_bytes) *lds_bytes = lds;
  if (blocks_per_cu) *blocks_per_cu = lds_blocks_per_cu(lds);
  if (wave_below) {
    const int w = spec_wave_below(wave_below_detector, 1, ty);
    *wave_below = w >= 0 ? w : wave_below_detector;
  }
  return CC_OK;
}

cc_status cc_debug_spec_step2_plan(const cc_cascade* c, int rows_wanted, int wave_below_detector, int* rows, size_t* lds_bytes, int* blocks_per_cu,
                                   int* wave_below) {
  if (!c) return set_error(CC_ERR_INVALID_ARG, "cc_debug_spec_step2_plan: null cascade");
  if (cc_status hs = refuse_hog(c->m, "cc_debug_spec_step2_plan"); hs != CC_OK) return hs;
  if (c->m.max_nodes_per_tree > 1 || !spec_lean_lds(c->m, TILE_32, 2))
    return set_error(CC_ERR_UNSUPPORTED, "cc_debug_spec_step2_plan: upright Haar stump cascades only");
  const int ty = rows_wanted > 0 ? rows_wanted : spec_step2_rows(c->m);
  if (ty < TILE_Y || ty > kSpecStep2MaxRows) return set_error(CC_ERR_INVALID_ARG, "cc_debug_spec_step2_plan: %d window rows per tile", ty);
  const size_t lds = spec_step2_lds(c->m, ty);
  if (rows) *rows = ty;
  if (lds_bytes) *lds_bytes = lds;
  if (blocks_per_cu) *blocks_per_cu = lds_blocks_resident(lds);
  if (wave_below) {
    const int w = spec_wave_below(wave_below_detector, 2, ty);
    *wave_below = w >= 0 ? w : wave_below_detector;
  }
  return CC_OK;
}

cc_status cc_cascade_compile_specialized(const cc_cascade* c, int n_stages, const char* arch, size_t* code_bytes) {
  if (!c || !arch || !code_bytes) return set_error(CC_ERR_INVALID_ARG, "cc_cascade_compile_specialized: null argument");
  if (cc_status hs = refuse_hog(c->m, "cc_cascade_compile_specialized"); hs != CC_OK) return hs;
  std::vector<SpecCode> code;
  int k = 0;
  int tmode = 0;
  const cc_status st = spec_build(c->m, std::max(1, n_stages), arch, code, k, tmode);
  if (st != CC_OK) return st;
  *code_bytes = 0;
  for (const SpecCode& m : code) *code_bytes += m.code.size();  // all modules (Haar: one per step)
  return CC_OK;
}

}  // extern "C"
