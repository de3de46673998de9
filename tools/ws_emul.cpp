// ws_emul.cpp -- development tool: replays hrf_watershed_ex's flow on the CPU, serially, with the
// kernels' own rules (csrc/ws_core.hpp: the relaxation's order, initial state and transition, the
// contest decision, the resolution), so they can be checked against the heap flood
// (oracle_watershed) without a GPU.  Not part of libhrf.so.
//   hipcc -O2 -fPIC -shared -o tools/libws_emul.so tools/ws_emul.cpp
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <vector>

#include "../hiprfish_image_analysis_amd/csrc/ws_core.hpp"

using namespace hrf_ws;

extern "C" int ws_emul(const double *f, int negate, const int32_t *mk, const uint8_t *mask, int64_t H, int64_t W,
                       int32_t *out, int32_t *ties, int32_t *ptr_out = nullptr, double *lam_out = nullptr,
                       int32_t *hop_out = nullptr) {
  const int64_t n = H * W;
  std::vector<double> lam(n);
  std::vector<int32_t> hop(n), lab(n), ptr(n, -1), dst(n);
  auto in = [&](int64_t i) { return !mask || mask[i]; };
  WsGeom g{f, negate, mk, mask, H, W, lam.data(), hop.data()};
  for (int64_t i = 0; i < n; ++i) {
    const WsCell c = ws_start(in(i), mk, f, negate, i);
    lam[i] = c.lam, hop[i] = c.hop, dst[i] = c.dst, lab[i] = c.lab;
  }
  for (bool ch = true; ch;) {  // relaxation, the pass kernels' rule (ws_core.hpp)
    ch = false;
    for (int64_t x = 0; x < n; ++x) {
      if (!in(x) || mk[x]) continue;
      int64_t nb[4];
      const int k = g_nbrs(g, x, nb);
      WsCell best = ws_free();
      for (int j = 0; j < k; ++j) {
        const int64_t y = nb[j];
        if (!lab[y] || !in(y)) continue;
        const WsCell c{lam[y], hop[y], dst[y], lab[y]};
        if (better(c, best)) best = c;
      }
      if (!best.lab) continue;
      const WsCell c = ws_step(best, g_f(g, x));
      if (c.lam != lam[x] || c.hop != hop[x] || c.dst != dst[x] || c.lab != lab[x]) {
        lam[x] = c.lam, hop[x] = c.hop, dst[x] = c.dst, lab[x] = c.lab;
        ch = true;
      }
    }
  }
  const int32_t capx = getenv("WS_EMUL_CAPX") ? atoi(getenv("WS_EMUL_CAPX")) : 16;
  const int32_t cap = getenv("WS_EMUL_SMALL") ? 4096 : (int32_t)(capx * n + 64),
                hcap = getenv("WS_EMUL_SMALL") ? 8192 : 1 << (int)std::ceil(std::log2(2.0 * (capx * n + 64))), gcap = cap;
  std::vector<int32_t> pa(cap), ga(cap), pb(cap), gb(cap), slots(cap), mh(gcap), mr(gcap);
  std::vector<uint64_t> hkey(hcap);
  std::vector<uint32_t> hgen(hcap, 0);
  std::vector<double> ml(gcap);
  std::vector<uint8_t> alive(gcap);
  Walker w{pa.data(), ga.data(), pb.data(), gb.data(), slots.data(), hkey.data(), hgen.data(), ml.data(),
           mh.data(), mr.data(), alive.data(), cap, hcap, gcap, 0, 0};
  int32_t total = 0, rounds = 0, layout = 0;
  for (;;) {
    std::vector<int32_t> list;
    for (int64_t x = 0; x < n; ++x) {
      if (!in(x) || mk[x] || lam[x] == INFINITY || ptr[x] >= 0) continue;
      if (ws_contested(g, x, lab.data())) list.push_back((int32_t)x);
    }
    if (list.empty()) break;
    total += (int32_t)list.size();
    ++rounds;
    if (getenv("WS_EMUL_CHECK")) {  // every listed basin pixel resolves its component alone
      std::vector<int32_t> ref(n, -1), tmp(n, -1);
      for (int32_t x : list) {
        if (!(!in(x) || mk[x]) && (negate ? -f[x] : f[x]) < lam[x]) {
          std::fill(tmp.begin(), tmp.end(), -1);
          int32_t lay = 0;
          if (!ws_resolve_one(g, x, tmp.data(), w, &lay)) return 3;
          for (int64_t i = 0; i < n; ++i)
            if (tmp[i] >= 0) {
              if (ref[i] >= 0 && ref[i] != tmp[i]) {
                fprintf(stderr, "inconsistent tree at %lld (from %d): %d vs %d\n", (long long)i, x, ref[i], tmp[i]);
              }
              ref[i] = tmp[i];
            }
        }
      }
    }
    if (getenv("WS_EMUL_ROOTS")) {
      std::vector<int32_t> tmp(n, -1);
      for (int32_t x : list) {
        int32_t lay = 0, rt = -1;
        ws_resolve_one(g, x, tmp.data(), w, &lay, &rt);
        fprintf(stderr, "emul: round %d resolve %d -> %d\n", rounds, x, rt);
      }
    }
    for (int32_t x : list) {
      if (ptr[x] >= 0) continue;
      if (!ws_resolve_one(g, x, ptr.data(), w, &layout)) return 1;
    }
    for (int64_t i = 0; i < n; ++i) lab[i] = in(i) ? mk[i] : 0;
    const bool jacobi = getenv("WS_EMUL_JACOBI") != nullptr;
    for (bool ch = true; ch;) {  // relabel, the RELABEL pass rule
      ch = false;
      std::vector<int32_t> old(lab);
      for (int64_t x = 0; x < n; ++x) {
        if (!in(x) || mk[x] || lam[x] == INFINITY) continue;
        int32_t lb = 0;
        const int32_t *src = jacobi ? old.data() : lab.data();
        if (ptr[x] >= 0) lb = src[ptr[x]];
        else {
          int32_t cc[4];
          const int m = g_cands(g, x, cc);
          for (int j = 0; j < m; ++j)
            if (src[cc[j]] && (!lb || src[cc[j]] < lb)) lb = src[cc[j]];
        }
        if (lb != lab[x]) {
          lab[x] = lb;
          ch = true;
        }
      }
    }
    if (rounds > 10000) return 2;
  }
  std::memcpy(out, lab.data(), sizeof(int32_t) * n);
  if (ptr_out) std::memcpy(ptr_out, ptr.data(), sizeof(int32_t) * n);
  if (lam_out) std::memcpy(lam_out, lam.data(), sizeof(double) * n);
  if (hop_out) std::memcpy(hop_out, hop.data(), sizeof(int32_t) * n);
  ties[0] = total;
  ties[1] = rounds;
  ties[2] = layout;
  return 0;
}
