// arena_sizes.h — the four sizes that both the kernels and the host's arena plan (host/context_layout.cc) need: one statement
// of each.  Plain C++, no HIP type: hipcc compiles the same text for the kernels (fd_kernel.h, trust_region.h, kernels.h
// include it), g++ for the host-only unit and tests/cpp/context_layout_check.cc.
#pragma once
#if defined(__HIPCC__)
#define IDTO_AS_HD __host__ __device__
#else
#define IDTO_AS_HD
#endif
namespace idto_dev {
// doubles of one record's assembly products (fd_kernel.h: CP, CT, CM lower triangles padded to nq x nq, BPT, BTM, APM, gP, gT,
// gM; + 1 where that is odd: 16-byte alignment)
IDTO_AS_HD inline int asm_terms_stride(int nq) { return 6 * nq * nq + 3 * nq + ((3 * nq) & 1); }
// sums per block row of the resident trust-region loop (trust_region.h TrPrepareArgs::part_ll)
constexpr int TR_NSUM = 10;
// state words of the resident trust-region loop (trust_region.h TRS_*)
enum { TRS_COUNT = 12 };
// spare records behind the slab's N: the in-place all-gather of a sharded run pads every rank's range (at most this many ranks)
enum { IDTO_SLAB_PAD = 64 };
}  // namespace idto_dev
