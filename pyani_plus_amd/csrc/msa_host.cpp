// msa_host.cpp -- host side of external-alignment-hip: the MSA file -> (md5, titles, rows, residue histogram), and the
// per-pair transform (M, B, n_q, n_s) -> the five numbers the reference reports.
//
// The reference parses the alignment twice per subject column with fasta_bytes_iterator
// (pyani_plus/methods/external_alignment.py:63-99, parser pyani_plus/utils.py:40-90) and checks the file's md5
// first (pyani_plus/private_cli.py:1985-1990).  Here the file is read once: the md5 runs on its own thread beside
// the parse, and the records are parsed in parallel once their '>' lines are known.  No gzip: the reference opens the
// alignment with plain open("rb").
//
// Parser semantics (fasta_bytes_iterator): the file is split at '\n'; lines before the first one that starts with
// '>' are skipped; a title is line[1:].rstrip(); every other line is rstrip()ed (ASCII whitespace: " \t\n\r\v\f"),
// the lines of a record are joined and every byte of " \t\r\n" is deleted.  Every other byte is a residue.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "pa_host.h"
#include "md5.h"

struct pa_msa {
  std::vector<uint8_t> seq;      // record i's residues at seq[seq0[i], seq0[i] + seq_len[i]) (seq0[i]: where its text starts)
  std::vector<std::string> titles;  // NUL-terminated, handed out by pa_msa_record
  std::vector<uint64_t> seq0, seq_len;
  uint64_t hist[256] = {0};
  char md5[33] = {0};
};

namespace {

inline bool py_space(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == 0x0b || c == 0x0c; }

// end of line[b, e) after bytes.rstrip()
inline uint64_t rstrip(const uint8_t *d, uint64_t b, uint64_t e) {
  while (e > b && py_space(d[e - 1])) --e;
  return e;
}

// The body of one record, text d[b, e) (the lines after its title), -> its residues at o[b, ...); returns the residue
// count and adds them to hist.
uint64_t parse_body(const uint8_t *d, uint8_t *o, uint64_t b, uint64_t e, uint64_t *hist) {
  uint64_t out = b;
  uint64_t p = b;
  while (p < e) {
    const uint8_t *nl = static_cast<const uint8_t *>(memchr(d + p, '\n', e - p));
    const uint64_t line_end = nl ? (uint64_t)(nl - d) : e;
    const uint64_t keep = rstrip(d, p, line_end);
    for (uint64_t i = p; i < keep; ++i) {
      const uint8_t c = d[i];
      if (c == ' ' || c == '\t' || c == '\r' || c == '\n') continue;
      o[out++] = c;
      ++hist[c];
    }
    p = line_end + 1;
  }
  return out - b;
}

int msa_load(const char *path, int threads, pa_msa **out) {
  if (!path || !out) { pa_set_error("pa_msa_load: null argument"); return PA_E_INVALID; }
  *out = nullptr;
  FILE *f = fopen(path, "rb");
  if (!f) { pa_set_error("cannot open %s", path); return PA_E_IO; }
  auto m = std::make_unique<pa_msa>();
  if (fseeko(f, 0, SEEK_END) != 0) { fclose(f); pa_set_error("cannot seek in %s", path); return PA_E_IO; }
  const off_t size = ftello(f);
  rewind(f);
  std::vector<uint8_t> text((size_t)std::max<off_t>(size, 0));
  const bool read_ok = text.empty() || fread(text.data(), 1, text.size(), f) == text.size();
  fclose(f);
  if (size < 0 || !read_ok) { pa_set_error("cannot read %s", path); return PA_E_IO; }
  const uint8_t *d = text.data();
  const uint64_t n = text.size();
  m->seq.resize(n);

  // md5 of the raw bytes on a thread of its own while the records are found and parsed (serial per file, and the
  // parse never writes to the text)
  Md5 md5;
  std::thread md5_thread([&] { md5.update(d, n); });
  struct Joiner {  // an exception of the parse (std::bad_alloc) never leaves a joinable thread behind
    std::thread &t;
    ~Joiner() { if (t.joinable()) t.join(); }
  } joiner{md5_thread};

  // every line that starts with '>': the first one ends the preamble, each one starts a record
  std::vector<uint64_t> gt;
  if (n && d[0] == '>') gt.push_back(0);
  for (uint64_t p = 0; p < n;) {
    const uint8_t *nl = static_cast<const uint8_t *>(memchr(d + p, '\n', n - p));
    if (!nl) break;
    p = (uint64_t)(nl - d) + 1;
    if (p < n && d[p] == '>') gt.push_back(p);
  }
  const uint32_t n_rec = (uint32_t)gt.size();
  if ((uint64_t)n_rec != gt.size()) { pa_set_error("%s: too many records", path); return PA_E_INVALID; }
  m->titles.resize(n_rec);
  m->seq0.resize(n_rec);
  m->seq_len.resize(n_rec);
  std::vector<uint64_t> body1(n_rec);
  for (uint32_t r = 0; r < n_rec; ++r) {
    const uint64_t t = gt[r];
    const uint8_t *nl = static_cast<const uint8_t *>(memchr(d + t, '\n', n - t));
    const uint64_t line_end = nl ? (uint64_t)(nl - d) : n;
    m->titles[r].assign(reinterpret_cast<const char *>(d + t + 1), rstrip(d, t + 1, line_end) - (t + 1));
    m->seq0[r] = std::min(n, line_end + 1);
    body1[r] = r + 1 < n_rec ? gt[r + 1] : n;
  }

  const uint32_t nt = pa_host_threads(n, 1u << 22, threads > 0 ? (uint32_t)threads : 0u);
  std::vector<std::array<uint64_t, 256>> hists(nt);
  for (auto &h : hists) h.fill(0);
  // records are handed out in order of a shared counter: one huge record and many small ones balance themselves
  pa_for_chunks(0, n_rec, 1, nt, [&](uint32_t w, uint64_t r, uint64_t) {
    m->seq_len[r] = parse_body(d, m->seq.data(), m->seq0[r], body1[r], hists[w].data());
  });
  md5_thread.join();
  md5.hex(m->md5);
  for (auto &h : hists)
    for (int c = 0; c < 256; ++c) m->hist[c] += h[c];
  *out = m.release();
  return PA_OK;
}

}  // namespace

extern "C" int pa_msa_load(const char *path, int threads, pa_msa **out) {
  return pa_host_guard("pa_msa_load", [&] { return msa_load(path, threads, out); });
}

extern "C" int pa_msa_info(const pa_msa *m, uint32_t *n_records, uint64_t *max_len, char md5hex33[33], uint64_t *h_hist256) {
  if (!m) { pa_set_error("pa_msa_info: null handle"); return PA_E_INVALID; }
  if (n_records) *n_records = (uint32_t)m->seq0.size();
  if (max_len) *max_len = m->seq_len.empty() ? 0 : *std::max_element(m->seq_len.begin(), m->seq_len.end());
  if (md5hex33) memcpy(md5hex33, m->md5, 33);
  if (h_hist256) memcpy(h_hist256, m->hist, sizeof(m->hist));
  return PA_OK;
}

extern "C" int pa_msa_record(const pa_msa *m, uint32_t i, const char **title, uint64_t *title_len, uint64_t *length) {
  if (!m || i >= m->seq0.size()) { pa_set_error("pa_msa_record: no record %u", i); return PA_E_INVALID; }
  if (title) *title = m->titles[i].c_str();
  if (title_len) *title_len = m->titles[i].size();
  if (length) *length = m->seq_len[i];
  return PA_OK;
}

// rows [r0, r1) into h_rows, row_stride bytes each: the residues, then '-' up to the stride (a shorter row's tail is
// gap); a row longer than the stride is an error
extern "C" int pa_msa_copy_rows(const pa_msa *m, uint32_t r0, uint32_t r1, uint64_t row_stride, uint8_t *h_rows) {
  if (!m || !h_rows || r0 > r1 || r1 > m->seq0.size()) { pa_set_error("pa_msa_copy_rows: bad arguments"); return PA_E_INVALID; }
  for (uint32_t r = r0; r < r1; ++r)
    if (m->seq_len[r] > row_stride) {
      pa_set_error("pa_msa_copy_rows: record %u has %llu residues, more than the row stride %llu", r, (unsigned long long)m->seq_len[r],
                   (unsigned long long)row_stride);
      return PA_E_INVALID;
    }
  return pa_host_guard("pa_msa_copy_rows", [&] {
    const uint32_t nt = pa_host_threads((uint64_t)(r1 - r0) * row_stride, 1u << 22, 0);
    HostPool::get().run(nt, [&](uint32_t w, uint32_t n_w) {
      for (uint32_t r = r0 + w; r < r1; r += n_w) {
        uint8_t *dst = h_rows + (uint64_t)(r - r0) * row_stride;
        memcpy(dst, m->seq.data() + m->seq0[r], m->seq_len[r]);
        memset(dst + m->seq_len[r], '-', row_stride - m->seq_len[r]);
      }
    });
    return PA_OK;
  });
}

extern "C" void pa_msa_free(pa_msa *m) { delete m; }

// (M, B, n_q, n_s) per pair -> the reference's five numbers (pyani_plus/methods/external_alignment.py:118-156):
//   aln_length = n_q + n_s - B, identity = M / aln_length, sim_errors = aln_length - M,
//   cov_query = B / n_q, cov_subject = B / n_s.
// The reference divides Python ints (correctly rounded); every operand here is below 2^53, so the IEEE double
// division of the converted operands is the same double.
extern "C" int pa_msa_metrics(const uint32_t *h_match, const uint32_t *h_both, const uint64_t *h_nq, const uint64_t *h_ns, uint64_t n_pairs,
                              double *h_identity, int64_t *h_aln_length, int64_t *h_sim_errors, double *h_cov_query,
                              double *h_cov_subject, uint32_t n_threads) {
  if (n_pairs && (!h_match || !h_both || !h_nq || !h_ns || !h_identity || !h_aln_length || !h_sim_errors || !h_cov_query || !h_cov_subject)) {
    pa_set_error("pa_msa_metrics: null argument");
    return PA_E_INVALID;
  }
  for (uint64_t i = 0; i < n_pairs; ++i)
    if (h_nq[i] == 0 || h_ns[i] == 0 || h_both[i] > h_nq[i] || h_both[i] > h_ns[i] || h_match[i] > h_both[i]) {
      pa_set_error("pa_msa_metrics: pair %llu has inconsistent counts (M %u, B %u, n_q %llu, n_s %llu)", (unsigned long long)i, h_match[i],
                   h_both[i], (unsigned long long)h_nq[i], (unsigned long long)h_ns[i]);
      return PA_E_INVALID;
    }
  return pa_host_guard("pa_msa_metrics", [&] {
    const uint32_t nt = pa_host_threads(n_pairs, 1u << 16, n_threads);
    HostPool::get().run(nt, [&](uint32_t w, uint32_t n_w) {
      const uint64_t lo = n_pairs * w / n_w, hi = n_pairs * (w + 1) / n_w;
      for (uint64_t i = lo; i < hi; ++i) {
        const uint64_t aln = h_nq[i] + h_ns[i] - h_both[i];
        h_aln_length[i] = (int64_t)aln;
        h_sim_errors[i] = (int64_t)(aln - h_match[i]);
        h_identity[i] = (double)h_match[i] / (double)aln;
        h_cov_query[i] = (double)h_both[i] / (double)h_nq[i];
        h_cov_subject[i] = (double)h_both[i] / (double)h_ns[i];
      }
    });
    return PA_OK;
  });
}
