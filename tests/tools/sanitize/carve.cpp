// The workspace carver (pa_carve.h: Carve, carve_measure, carve_place) under AddressSanitizer / UBSan: a stand-alone CPU
// program, no HIP runtime.  Every layout is placed on a heap block of exactly the measured size and every part is
// written in full, so a part that leaves its allocation trips the sanitizer.
//   usage: carve
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../../pyani_plus_amd/csrc/pa_carve.h"

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("MISMATCH %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                    \
    }                                                                \
  } while (0)

struct Wide {  // 16 bytes on 8, as nj_rule.h's Cand
  double q;
  uint32_t lo, hi;
};

// A layout as data: parts of a kind (the size of its type: 1, 2, 4, 8, or 16 for Wide; 0: slack of `count` bytes)
struct Part {
  uint32_t kind;
  uint64_t count, align;  // align 0: the type's own
};
struct Placed {
  char *at;
  uint64_t bytes, align;
};

static Placed take(Carve &k, const Part &p) {
  switch (p.kind) {
    case 0: k.slack(p.count); return {nullptr, p.count, 0};
    case 1: return {reinterpret_cast<char *>(p.align ? k.take<uint8_t>(p.count, p.align) : k.take<uint8_t>(p.count)), p.count, p.align ? p.align : 1};
    case 2: return {reinterpret_cast<char *>(p.align ? k.take<uint16_t>(p.count, p.align) : k.take<uint16_t>(p.count)), p.count * 2, p.align ? p.align : 2};
    case 4: return {reinterpret_cast<char *>(p.align ? k.take<uint32_t>(p.count, p.align) : k.take<uint32_t>(p.count)), p.count * 4, p.align ? p.align : 4};
    case 8: return {reinterpret_cast<char *>(p.align ? k.take<uint64_t>(p.count, p.align) : k.take<uint64_t>(p.count)), p.count * 8, p.align ? p.align : 8};
    default: return {reinterpret_cast<char *>(p.align ? k.take<Wide>(p.count, p.align) : k.take<Wide>(p.count)), p.count * 16, p.align ? p.align : alignof(Wide)};
  }
}

static void *block_of(uint64_t bytes, uint64_t align) {
  void *p = nullptr;
  if (posix_memalign(&p, align < sizeof(void *) ? sizeof(void *) : align, bytes) != 0) abort();
  return p;
}

// Measures, places on a block of exactly the measured bytes, writes every part, and checks the properties of a good
// layout; `want_offsets` (optional) are the parts' expected offsets, slack excluded.  Returns the measured bytes.
static uint64_t run_layout(const std::vector<Part> &parts, const std::vector<uint64_t> &want_offsets = {}) {
  std::vector<Placed> placed;
  auto layout = [&](Carve &k) {
    placed.clear();
    for (const Part &p : parts) placed.push_back(take(k, p));
  };
  uint64_t measured = 0;
  CHECK(carve_measure(layout, &measured) == CarveVerdict::kOk);
  for (const Placed &q : placed) CHECK(q.at == nullptr);  // the measuring pass hands out nothing
  uint64_t max_align = 1;
  for (const Placed &q : placed) max_align = q.align > max_align ? q.align : max_align;
  char *base = static_cast<char *>(block_of(measured, max_align));
  CHECK(carve_place(base, measured, layout) == CarveVerdict::kOk);
  uint64_t end = 0, trailing_slack = 0, n_seen = 0;
  for (const Placed &q : placed) {
    if (q.align == 0) {  // slack
      trailing_slack += q.bytes;
      continue;
    }
    const uint64_t off = (uint64_t)(q.at - base);
    CHECK(q.at != nullptr && off >= end + trailing_slack);                  // after everything before it: no overlap
    CHECK(off - (end + trailing_slack) < q.align);                          // and no further than its alignment asks
    CHECK(reinterpret_cast<uintptr_t>(q.at) % q.align == 0);
    if (!want_offsets.empty()) CHECK(n_seen < want_offsets.size() && want_offsets[n_seen] == off);
    ++n_seen;
    memset(q.at, 0xA5, q.bytes);
    end = off + q.bytes;
    trailing_slack = 0;
  }
  CHECK(measured == end + trailing_slack);
  if (!want_offsets.empty()) CHECK(n_seen == want_offsets.size());
  free(base);
  return measured;
}

int main() {
  // an empty layout, and one part
  CHECK(run_layout({}) == 0);
  CHECK(run_layout({{4, 7, 0}}, {0}) == 28);
  CHECK(run_layout({{4, 0, 0}}, {0}) == 0);
  // parts of count 0 at the start, the middle and the end: each has an offset, none has bytes
  CHECK(run_layout({{8, 0, 0}, {4, 3, 0}, {16, 0, 0}, {1, 5, 0}, {8, 0, 0}}, {0, 0, 16, 16, 24}) == 24);
  // u8, u64, u32: padding appears (7 bytes before the u64) and then disappears
  CHECK(run_layout({{1, 1, 0}, {8, 2, 0}, {4, 3, 0}}, {0, 8, 24}) == 36);
  // explicit alignments 16 and 64
  CHECK(run_layout({{4, 1, 0}, {16, 2, 16}, {1, 3, 0}, {8, 1, 64}, {4, 1, 16}}, {0, 16, 48, 64, 80}) == 84);
  CHECK(run_layout({{1, 32, 32}, {4, 8, 0}}, {0, 32}) == 64);
  // slack between parts and at the end
  CHECK(run_layout({{8, 4, 0}, {0, 32, 0}, {8, 3, 0}, {0, 16, 0}}, {0, 64}) == 104);
  CHECK(run_layout({{4, 3, 0}, {0, 1, 0}, {4, 1, 0}, {0, 5, 0}}, {0, 16}) == 25);
  // slack alone
  CHECK(run_layout({{0, 16, 0}}) == 16);

  // align_to says what it skipped, and the layout of nj.hip's tail follows from it: 16 bytes set aside, the part on 16
  for (uint64_t lead = 0; lead < 40; lead += 4) {
    uint64_t measured = 0;
    char *cand = nullptr;
    auto layout = [&](Carve &k) {
      k.take<uint32_t>(lead / 4);
      const uint64_t skipped = k.align_to(16);
      cand = reinterpret_cast<char *>(k.take<Wide>(3, 16));
      k.slack(16 - skipped);
    };
    CHECK(carve_measure(layout, &measured) == CarveVerdict::kOk && measured == lead + 16 + 3 * sizeof(Wide));
    char *base = static_cast<char *>(block_of(measured, 16));
    CHECK(carve_place(base, measured, layout) == CarveVerdict::kOk);
    CHECK((uint64_t)(cand - base) == ((lead + 15) & ~15ull));
    memset(base, 0, measured);
    free(base);
  }

  // sizes that do not fit 64 bits are refused, not wrapped: a count times its type's size, and the running offset
  {
    uint64_t measured = 0;
    CHECK(carve_measure([](Carve &k) { k.take<uint64_t>((1ull << 61) + 1); }, &measured) == CarveVerdict::kTooLarge);
    CHECK(carve_measure([](Carve &k) { k.take<Wide>(1ull << 60); }, &measured) == CarveVerdict::kTooLarge);
    CHECK(carve_measure([](Carve &k) { k.take<uint64_t>((1ull << 61) - 1); }, &measured) == CarveVerdict::kOk && measured == ~0ull - 7);
    CHECK(carve_measure([](Carve &k) { k.take<uint8_t>(~0ull - 2); k.take<uint32_t>(0); }, &measured) == CarveVerdict::kTooLarge);  // the padding wraps
    CHECK(carve_measure([](Carve &k) { k.take<uint8_t>(~0ull - 4); k.take<uint8_t>(8); }, &measured) == CarveVerdict::kTooLarge);
    CHECK(carve_measure([](Carve &k) { k.take<uint8_t>(~0ull - 4); k.slack(5); }, &measured) == CarveVerdict::kTooLarge);
    CHECK(carve_measure([](Carve &k) { k.take<uint8_t>(~0ull - 4); k.slack(4); }, &measured) == CarveVerdict::kOk && measured == ~0ull);
    // the refusal sticks: what follows it is not handed out and does not move the end
    Carve k;
    k.take<uint64_t>(4);
    k.take<uint64_t>(1ull << 62);
    CHECK(k.verdict() == CarveVerdict::kTooLarge && k.end() == 32);
    k.take<uint32_t>(1);
    CHECK(k.verdict() == CarveVerdict::kTooLarge && k.end() == 32);
    // an alignment that is no power of two, or below the type's own
    CHECK(carve_measure([](Carve &k) { k.take<uint32_t>(1, 24); }, &measured) == CarveVerdict::kBadAlignment);
    CHECK(carve_measure([](Carve &k) { k.take<uint64_t>(1, 4); }, &measured) == CarveVerdict::kBadAlignment);
    CHECK(carve_measure([](Carve &k) { k.take<uint64_t>(1, 0); }, &measured) == CarveVerdict::kBadAlignment);
    CHECK(carve_measure([](Carve &k) { k.align_to(0); }, &measured) == CarveVerdict::kBadAlignment);
  }

  // a base that is misaligned for the largest alignment asked is refused, whichever part asked it
  {
    uint32_t *first = nullptr;
    uint8_t *second = nullptr;
    auto layout = [&](Carve &k) {
      first = k.take<uint32_t>(4);
      second = k.take<uint8_t>(64, 64);
    };
    uint64_t measured = 0;
    CHECK(carve_measure(layout, &measured) == CarveVerdict::kOk && measured == 128);
    char *block = static_cast<char *>(block_of(measured + 16, 64));
    CHECK(carve_place(block + 16, measured, layout) == CarveVerdict::kMisaligned);
    CHECK(carve_place(block, measured, layout) == CarveVerdict::kOk && reinterpret_cast<char *>(second) == block + 64);
    auto tail_only = [&](Carve &k) { k.take<uint32_t>(4); k.align_to(64); };  // asked by no part: the base still answers for it
    CHECK(carve_measure(tail_only, &measured) == CarveVerdict::kOk && measured == 64);
    CHECK(carve_place(block + 16, measured, tail_only) == CarveVerdict::kMisaligned);
    free(block);
  }

  // two passes that disagree: the layout reads a variable that changed in between
  {
    uint64_t n = 10, measured = 0;
    uint32_t *a = nullptr, *b = nullptr;
    auto layout = [&](Carve &k) {
      a = k.take<uint32_t>(n);
      b = k.take<uint32_t>(n);
    };
    CHECK(carve_measure(layout, &measured) == CarveVerdict::kOk && measured == 80);
    char *base = static_cast<char *>(block_of(measured, 8));
    n = 11;  // larger: the second part would leave the block; it is refused before its address is formed
    CHECK(carve_place(base, measured, layout) == CarveVerdict::kPassesDisagree);
    CHECK(b == nullptr);
    n = 9;  // smaller: everything fits, the end differs
    CHECK(carve_place(base, measured, layout) == CarveVerdict::kPassesDisagree);
    n = 10;
    CHECK(carve_place(base, measured, layout) == CarveVerdict::kOk && reinterpret_cast<char *>(b) == base + 40);
    memset(a, 0, 40);
    memset(b, 0, 40);
    free(base);
    // a layout of nothing placed on no allocation (a buffer that never had to grow)
    CHECK(carve_place(nullptr, 0, [](Carve &k) { CHECK(k.take<uint64_t>(0) == nullptr); }) == CarveVerdict::kOk);
  }

  // 1 000 random part lists from a fixed seed
  std::mt19937_64 rng(20240607);
  const uint32_t kinds[6] = {0, 1, 2, 4, 8, 16};
  const uint64_t aligns[4] = {0, 0, 16, 64};
  for (int trial = 0; trial < 1000; ++trial) {
    std::vector<Part> parts(rng() % 9);
    for (Part &p : parts) {
      p.kind = kinds[rng() % 6];
      p.count = rng() % 4 == 0 ? 0 : rng() % 41;
      p.align = p.kind ? aligns[rng() % 4] : 0;
    }
    run_layout(parts);
  }

  if (failures) return 1;
  printf("workspace layouts agree\n");
  return 0;
}
