// strict_fp.h -- contraction off, from this include to the end of the translation unit: a product is rounded before it
// is added, on the device (hipcc's default is -ffp-contract=fast) and on the host (a host compiler contracts once FMA
// instructions are enabled).  Every header that states bit-exact arithmetic includes this itself, so that it cannot be
// included the wrong way round; a source file whose own arithmetic is bit-exact includes it as well.  The Makefile's
// STRICT_FP list passes -ffp-contract=off for the same files, as the second line of defence: -ffp-contract=fast on a
// clang command line would override the pragma, and no target passes that.
#pragma once

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif
