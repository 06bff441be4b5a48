// pa_host.h -- what a host translation unit opens with: the C interface, the host pool and its work-sharing loop, the
// error message of the calling thread, and the guard of an entry point's body.
#pragma once

#include <exception>
#include <new>

#include "../../include/pyani_hip.h"
#include "host_pool.h"

// printf-style; the message pa_last_error returns on this thread (capi.hip; a stand-alone test program defines its own)
void pa_set_error(const char *fmt, ...);

// Body of an extern "C" entry point that runs host-pool jobs or allocates: C++ exceptions never cross the C ABI.
// Returns the body's status, PA_E_NOMEM for std::bad_alloc, PA_E_INVALID for anything else, with the message set.
template <typename Body>
inline int pa_host_guard(const char *what, Body &&body) {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    pa_set_error("%s: out of host memory", what);
    return PA_E_NOMEM;
  } catch (const std::exception &e) {
    pa_set_error("%s: %s", what, e.what());
    return PA_E_INVALID;
  } catch (...) {
    pa_set_error("%s: unknown C++ exception", what);
    return PA_E_INVALID;
  }
}
