// The index maps of cddp-cpp_amd/csrc/io_layout.hpp -- the ones the device I/O kernels address the handle's buffers with -- against a
// direct restatement of the three layouts (dev_types.hpp; the slot rule of the slotted fields; kernels.hpp::GT).  The program tiles and
// un-tiles on the host THROUGH the maps and compares every (b, t, e) with the formulas written out here.  Built with
// -fsanitize=address,undefined by tests/test_device_io_layout.py: an index outside a buffer sized by the layout's own extent is a report.
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../../cddp-cpp_amd/csrc/io_layout.hpp"

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { if (fails < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

// a value that names its (b, t, e)
static double tag(int b, int t, int e) { return 1.0 + b * 1000003.0 + t * 1009.0 + e; }

static void run(int B, int T, int E) {
  const int Bp = (B + 63) / 64 * 64, NB = Bp / 64;
  const size_t n_stack = (size_t)T * E * Bp;
  std::vector<double> bm((size_t)B * T * E);
  for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int e = 0; e < E; ++e) {
    const size_t i = cddp_io::batch_major(b, T, t, E, e);
    EXPECT(i == ((size_t)b * T + t) * E + e);
    bm[i] = tag(b, t, e);
  }
  // wave-tiled: tile through the map, padding lanes left 0.0; every address is hit once
  {
    std::vector<double> st(n_stack, 0.0);
    std::vector<char> hit(n_stack, 0);
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int e = 0; e < E; ++e) {
      const size_t a = cddp_io::tiled(t, NB, E, e, b);
      EXPECT(a == ((((size_t)t * NB + (size_t)(b / 64)) * E + e) * 64 + (size_t)(b % 64)));
      EXPECT(a < n_stack && !hit[a]);
      if (a < n_stack) { hit[a] = 1; st.at(a) = bm[cddp_io::batch_major(b, T, t, E, e)]; }
    }
    for (int b = B; b < Bp; ++b) for (int t = 0; t < T; ++t) for (int e = 0; e < E; ++e) {   // the padding lanes of the last tile
      const size_t a = cddp_io::tiled(t, NB, E, e, b);
      EXPECT(a < n_stack && !hit[a] && st.at(a) == 0.0);
    }
    std::vector<double> back((size_t)B * T * E, -1.0);
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int e = 0; e < E; ++e)
      back[cddp_io::batch_major(b, T, t, E, e)] = st.at(cddp_io::internal(cddp_io::kTiled, 0, 0, t, NB, E, e, b));
    EXPECT(back == bm);
  }
  // sub-tile-minor
  {
    std::vector<double> st(n_stack, 0.0);
    std::vector<char> hit(n_stack, 0);
    const size_t NB16 = (size_t)NB * 16;
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int e = 0; e < E; ++e) {
      const size_t a = cddp_io::t4(t, NB, E, e, b);
      EXPECT(a == ((((size_t)t * NB16 + (size_t)(b / 4)) * (size_t)E + (size_t)e) * 4 + (size_t)(b % 4)));
      EXPECT(a < n_stack && !hit[a]);
      if (a < n_stack) { hit[a] = 1; st.at(a) = tag(b, t, e); }
    }
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int e = 0; e < E; ++e)
      EXPECT(st.at(cddp_io::internal(cddp_io::kT4, 0, 0, t, NB, E, e, b)) == tag(b, t, e));
  }
  // slotted: n_slots planes, the live slot scrambled per trajectory; the other planes hold a poison value
  {
    const int n_slots = 5;
    const size_t plane = n_stack;
    std::vector<double> st(plane * n_slots, -7.0);
    std::vector<int> cur(B);
    for (int b = 0; b < B; ++b) cur[b] = (b * 7 + 3) % n_slots;
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int e = 0; e < E; ++e) {
      const size_t a = cddp_io::slotted(cur[b], plane, t, NB, E, e, b);
      EXPECT(a == (size_t)cur[b] * plane + ((((size_t)t * NB + (size_t)(b / 64)) * E + e) * 64 + (size_t)(b % 64)));
      EXPECT(a < st.size());
      if (a < st.size()) st.at(a) = tag(b, t, e);
    }
    int wrong = 0;
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int e = 0; e < E; ++e)
      wrong += st.at(cddp_io::internal(cddp_io::kSlotted, cur[b], plane, t, NB, E, e, b)) != tag(b, t, e);
    EXPECT(wrong == 0);
    if (B > 1 && n_slots > 1) {   // the slot matters: read through a wrong slot and the poison comes back
      const int b = B - 1, other = (cur[b] + 1) % n_slots;
      EXPECT(st.at(cddp_io::slotted(other, plane, 0, NB, E, 0, b)) == -7.0);
    }
  }
}

int main() {
  const int shapes[][3] = {{1, 1, 1}, {64, 3, 2}, {70, 6, 9}, {130, 5, 4}};
  for (const auto &s : shapes) run(s[0], s[1], s[2]);
  // indices past 2^31 do not wrap: a stack of 3 * 2^28 doubles per step
  EXPECT(cddp_io::tiled(5, 1 << 20, 12, 11, (1 << 26) - 1) == ((((size_t)5 * (1u << 20) + ((1u << 20) - 1)) * 12 + 11) * 64 + 63));
  if (fails == 0) std::printf("io layout: ok\n");
  return fails == 0 ? 0 : 1;
}
