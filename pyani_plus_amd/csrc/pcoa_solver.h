// pcoa_solver.h -- the eigen-solver of ordinate-run as pcoa_host.cpp compiles it, for its two callers: pa_symm_top_eigs
// (pcoa.hip, the product on the device) and pa_symm_top_eigs_host (the product's host twin).  Everything but the product
// is this one piece of host code, so the two entry points differ by the product alone.
#pragma once

#include <cstdint>
#include <functional>

namespace pcoa {

// Y = B Q for the n x p row-major block Q; returns a PA_* status (its message already set)
using Product = std::function<int(const double *h_Q, uint32_t p, double *h_Y)>;

// The contract of pa_symm_top_eigs (include/pyani_hip.h); `what` names the entry point in messages.  Checks every
// argument but the matrix, which only `product` sees.
int top_eigs(const char *what, uint32_t n, uint32_t k, double tol, uint32_t max_iter, double fro2, const Product &product, double *h_values,
             double *h_vectors, double *h_residuals, double *h_info);

}  // namespace pcoa
