// distmat_host.cpp -- the check of a distance matrix on the host and the one message of its refusal, which the device
// check (distmat.hip) ends in too.  distmat_rule.h has the rule of a cell.
#include <cstdint>

#include "pa_host.h"
#include "distmat_rule.h"

int distmat::refuse(const char *who, const char *name, uint32_t n, uint64_t bad, uint64_t first) {
  pa_set_error("%s: %s[%llu,%llu] is not finite, is negative, differs from its transpose's bits or is a non-zero diagonal cell (%llu such cells)", who,
               name, (unsigned long long)(first / n), (unsigned long long)(first % n), (unsigned long long)bad);
  return PA_E_INVALID;
}

int pa_check_distance_matrix_host(const char *who, const char *name, const double *M, uint32_t n) {
  const uint64_t N = n;
  uint64_t bad = 0, first = 0;
  for (uint64_t i = 0; i < N; ++i)
    for (uint64_t j = 0; j < N; ++j)
      if (distmat::bad_cell(M[i * N + j], M[j * N + i], i == j) && bad++ == 0) first = i * N + j;
  return bad ? distmat::refuse(who, name, n, bad, first) : PA_OK;
}
