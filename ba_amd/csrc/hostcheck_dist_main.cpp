// Stand-alone driver of the derived tables of the distributed solve (dist_plan.h through ba_hostcheck_dist_tables
// of hostcheck.cpp), for a sanitizer build:
//   make -C ba_amd/csrc ../lib/hostcheck_dist_asan && ba_amd/lib/hostcheck_dist_asan
// The grid of tests/test_dist_tables.py: 5 / 8 / 9 / 13 tiles, panels of 2 / 3 / 4, the seven (ranks, layout) pairs,
// dense / band / arrow / two seeded random factor patterns, three ways of dealing the S pattern to the ranks.  Every
// op of the tap runs on every plan with output buffers of exactly the size it fills; the rectangles rank a sends to
// rank b must be those b receives from a, and a lowered limit must refuse.  Prints the counts and "ok".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

extern "C" int64_t ba_hostcheck_dist_tables(int op, const uint32_t* hdr, const char* layout, const uint8_t* nzL, const uint8_t* nz2,
                                            const uint64_t* bits, const int64_t* arg, int64_t* out, uint64_t cap, char* msg,
                                            uint32_t msg_cap);
extern "C" uint64_t ba_hostcheck_tile_factor(uint32_t nt, uint8_t* nz);

static int fail(const char* what) {
  fprintf(stderr, "hostcheck_dist: %s\n", what);
  return 1;
}

static unsigned long tables = 0;   // tap calls that filled an exact buffer
static uint64_t rng_state = 1;
static uint32_t rnd() {   // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 2685821237ull) >> 33);
}

struct Case {
  uint32_t hdr[4];   // nblk G N rank
  const char* layout;
};

// one op into a buffer of exactly the size it needs: first with one slot too few (must say so), then exact
static int run(int op, const Case& c, const uint8_t* nzL, const uint8_t* nz2, const uint64_t* bits, const int64_t* arg,
               std::vector<int64_t>* out, char* msg, uint32_t msg_cap) {
  std::vector<int64_t> big((size_t)16 * c.hdr[0] * c.hdr[0] * c.hdr[2] + 8192);
  const int64_t n = ba_hostcheck_dist_tables(op, c.hdr, c.layout, nzL, nz2, bits, arg, big.data(), big.size(), msg, msg_cap);
  if (n < 0) return fail("a table was refused");
  out->assign((size_t)n, 0);
  if (n > 0) {
    std::vector<int64_t> small((size_t)n - 1);
    if (ba_hostcheck_dist_tables(op, c.hdr, c.layout, nzL, nz2, bits, arg, small.data(), small.size(), nullptr, 0) != -3)
      return fail("a short buffer was not refused");
  }
  if (ba_hostcheck_dist_tables(op, c.hdr, c.layout, nzL, nz2, bits, arg, out->data(), out->size(), msg, msg_cap) != n)
    return fail("the exact buffer");
  ++tables;
  return 0;
}

int main() {
  const uint32_t nblks[] = {5, 8, 9, 13}, widths[] = {2, 3, 4};
  const struct { uint32_t n; const char* layout; } lays[] = {{1, nullptr}, {2, "tri"}, {3, "grid"}, {4, "grid"}, {8, "tri"},
                                                              {3, "col"}, {3, "row"}};
  unsigned long plans = 0, rects = 0, refusals = 0;
  for (uint32_t nblk : nblks)
    for (int pat = 0; pat < 5; ++pat) {
      // S pattern and its factor pattern
      std::vector<uint8_t> S((size_t)nblk * nblk, 0);
      rng_state = 1000ull * nblk + pat + 1;
      for (uint32_t i = 0; i < nblk; ++i)
        for (uint32_t k = 0; k <= i; ++k)
          S[(size_t)i * nblk + k] = i == k || pat == 0 || (pat == 1 && i - k <= 2) || (pat == 2 && i == nblk - 1) || (pat >= 3 && rnd() % 4 == 0);
      std::vector<uint8_t> F = S;
      ba_hostcheck_tile_factor(nblk, F.data());
      for (const auto& lay : lays)
        for (uint32_t G : widths)
          for (int deal = 0; deal < 3; ++deal) {
            const uint32_t N = lay.n;
            const size_t words = ((size_t)nblk * nblk + 63) / 64;
            // local patterns: bands along the diagonal / everything / random non-empty sets of ranks; always the diagonal
            std::vector<std::vector<uint8_t>> local(N, std::vector<uint8_t>((size_t)nblk * nblk, 0));
            std::vector<uint64_t> bits(words * N, 0);
            for (uint32_t i = 0; i < nblk; ++i)
              for (uint32_t k = 0; k <= i; ++k) {
                if (!S[(size_t)i * nblk + k]) continue;
                const uint32_t set = deal == 0 ? 1u << (i * N / nblk) : deal == 1 ? (1u << N) - 1 : 1 + rnd() % ((1u << N) - 1);
                for (uint32_t r = 0; r < N; ++r)
                  if ((set >> r & 1u) || i == k) {
                    const size_t b = (size_t)i * nblk + k;
                    local[r][b] = 1;
                    bits[r * words + (b >> 6)] |= 1ull << (b & 63);
                  }
              }
            std::vector<std::vector<int64_t>> ex(N);
            for (uint32_t r = 0; r < N; ++r) {
              const Case c = {{nblk, G, N, r}, lay.layout};
              std::vector<int64_t> o;
              char msg[128];
              const int64_t none[4] = {-1, 0, 0, 0};
              for (int op : {0, 1, 5, 7}) {
                if (run(op, c, F.data(), nullptr, nullptr, none, &o, msg, sizeof(msg))) return 1;
              }
              if (run(2, c, F.data(), S.data(), nullptr, none, &o, msg, sizeof(msg)) || run(2, c, nullptr, nullptr, nullptr, none, &o, msg, sizeof(msg)))
                return 1;
              if (run(4, c, F.data(), local[r].data(), nullptr, none, &o, msg, sizeof(msg))) return 1;
              if (o.size() != (size_t)nblk * nblk) return fail("the assembly map's size");
              for (uint32_t J = 0; J * G < nblk; ++J) {
                const int64_t a1[4] = {(int64_t)std::min(J * G + 2 * G, nblk), (int64_t)(J * G), (int64_t)std::min(J * G + G, nblk), 0};
                if (run(6, c, F.data(), nullptr, nullptr, a1, &o, msg, sizeof(msg))) return 1;
              }
              if (run(3, c, F.data(), nullptr, bits.data(), none, &ex[r], msg, sizeof(msg))) return 1;
              if (ex[r][0] != 0 || msg[0]) return fail("a refusal at the default limit");
              rects += (unsigned long)(ex[r][1] + ex[r][2]);
              if (ex[r][1] + ex[r][2]) {   // a limit one rectangle cannot meet: refused, the message cut to the buffer
                const int64_t low[4] = {64 * 64 - 1, 0, 0, 0};
                char cut[24];
                if (run(3, c, F.data(), nullptr, bits.data(), low, &o, cut, sizeof(cut))) return 1;
                if (o[0] != 1 || strncmp(cut, "sparse exchange of S: m", sizeof(cut)) != 0) return fail("the refusal");
                ++refusals;
              }
            }
            // a -> b as a sends it  ==  a -> b as b expects it
            auto list = [&](uint32_t r, bool recv, uint32_t peer) {
              const std::vector<int64_t>& t = ex[r];
              const size_t first = 3 + (recv ? N + 1 : 0), base = 3 + 4 * (size_t)(N + 1) + (recv ? 4 * (size_t)t[1] : 0);
              std::vector<int64_t> v;
              for (int64_t q = t[first + peer]; q < t[first + peer + 1]; ++q)
                v.insert(v.end(), t.begin() + base + 4 * q, t.begin() + base + 4 * q + 3);
              return v;
            };
            for (uint32_t a = 0; a < N; ++a)
              for (uint32_t b = 0; b < N; ++b) {
                if (a == b ? !list(a, false, a).empty() || !list(a, true, a).empty() : list(a, false, b) != list(b, true, a))
                  return fail("the exchange is not symmetric");
              }
            ++plans;
          }
    }
  printf("dist tables: %lu plans, %lu tables, %lu rectangles matched, %lu refusals: ok\n", plans, tables, rects, refusals);
  return 0;
}
