// The shared host pool under ThreadSanitizer: two callers at once (the FASTA loader works on a background thread
// while the main thread transforms or writes), many short jobs, results checked; then the pool's work-sharing loop
// (ChunkQueue, pa_for_chunks, pa_for_each) over the ranges its users hand it.   usage: pool_race [rounds]
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../../pyani_plus_amd/csrc/host_pool.h"

namespace {

struct Range {
  const char *what;
  uint64_t first, last, chunk;
};

// the rows that have a pair of their own among n rows, [0, n - 1), as pa_rowdist_euclid_host and pa_nj_host hand them
// out: they return before the loop for n < 2, so the range never wraps
Range pair_rows(const char *what, uint64_t n) { return Range{what, 0, n < 2 ? 0 : n - 1, 1}; }

// Every index of the range visited exactly once and none outside it, every chunk inside the range and no longer than
// `chunk`.  The counts are plain integers: the end of a job is what makes them the caller's to read, and an index
// handed out twice would also be a race for ThreadSanitizer to report.
long check_range(const Range &r, uint32_t workers) {
  const uint64_t len = r.last > r.first ? r.last - r.first : 0, chunk = r.chunk ? r.chunk : 1;
  long wrong = 0;
  std::atomic<long> outside{0};
  std::vector<uint32_t> seen(len);
  auto visit = [&](uint64_t i0, uint64_t i1) {
    if (!(r.first <= i0 && i0 < i1 && i1 <= r.last && i1 - i0 <= chunk)) { ++outside; return; }
    for (uint64_t i = i0; i < i1; ++i) ++seen[i - r.first];
  };
  auto settle = [&](const char *form) {
    long bad = outside.exchange(0);
    for (auto &s : seen) { bad += s != 1; s = 0; }
    if (bad) printf("%s, %u workers, %s: %ld indices not visited exactly once\n", r.what, workers, form, bad);
    wrong += bad;
  };
  pa_for_chunks(r.first, r.last, r.chunk, workers, [&](uint32_t w, uint64_t i0, uint64_t i1) {
    if (w >= std::max(workers, 1u)) ++outside;
    visit(i0, i1);
  });
  settle("pa_for_chunks");
  pa_for_each(r.first, r.last, r.chunk, workers, [&](uint64_t i) { visit(i, i + 1); });
  settle("pa_for_each");
  // a loop with state of its own per thread: the queue inside the job, the state added up afterwards
  std::vector<uint64_t> taken(std::max(workers, 1u), 0);
  ChunkQueue queue(r.first, r.last, r.chunk);
  HostPool::get().run(workers, [&](uint32_t w, uint32_t) {
    uint64_t mine = 0;
    for (uint64_t i0, i1; queue.take(i0, i1);) { visit(i0, i1); mine += i1 - i0; }
    taken[w] = mine;
  });
  uint64_t total = 0;
  for (uint64_t t : taken) total += t;
  if (total != len) ++outside;
  settle("ChunkQueue");
  return wrong;
}

long check_chunk_loops() {
  const Range ranges[] = {
      {"empty at 0", 0, 0, 1},
      {"empty at 5", 5, 5, 4},
      {"reversed", 7, 3, 2},
      pair_rows("pair rows of 0", 0),
      pair_rows("pair rows of 1", 1),
      pair_rows("pair rows of 2", 2),
      pair_rows("pair rows of 100", 100),
      {"one index", 0, 1, 16},
      {"from 13, one at a time", 13, 13 + 29, 1},
      {"length no multiple of the chunk", 3, 3 + 1000, 64},
      {"length a multiple of the chunk", 0, 1024, 16},
      {"chunk longer than the range", 2, 9, 64},
      {"chunk 0 counts as 1", 0, 5, 0},
      {"across 2^32", (1ull << 32) - 100, (1ull << 32) + 100, 64},
  };
  long wrong = 0;
  for (const Range &r : ranges)
    for (uint32_t workers : {1u, 2u, 7u}) wrong += check_range(r, workers);
  return wrong;
}

}  // namespace

int main(int argc, char **argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 2000;
  std::atomic<long> wrong{0};
  auto caller = [&](uint32_t workers, int salt) {
    std::vector<long> slots(workers);
    for (int r = 0; r < rounds; ++r) {
      for (auto &s : slots) s = 0;
      HostPool::get().run(workers, [&](uint32_t w, uint32_t n) {
        if (n != workers) ++wrong;
        slots[w] += (long)(w + 1) * (r + salt);
      });
      for (uint32_t w = 0; w < workers; ++w)
        if (slots[w] != (long)(w + 1) * (r + salt)) ++wrong;
    }
  };
  std::thread a(caller, 4u, 1), b(caller, 7u, 1000), c(caller, 2u, 5);
  a.join();
  b.join();
  c.join();
  printf("budget %u threads; %d rounds x 3 callers, wrong results: %ld\n", pa_cpu_budget(), rounds, wrong.load());
  // the work-sharing loop: from one caller, then from two at once (one of them gets the pool, the other threads of its own)
  std::atomic<long> wrong_chunks{check_chunk_loops()};
  std::thread d([&] { wrong_chunks += check_chunk_loops(); }), e([&] { wrong_chunks += check_chunk_loops(); });
  d.join();
  e.join();
  printf("chunk loops: 14 ranges x 3 worker counts x 3 forms, alone and from two callers at once, wrong indices: %ld\n", wrong_chunks.load());
  return wrong.load() || wrong_chunks.load() ? 1 : 0;
}
