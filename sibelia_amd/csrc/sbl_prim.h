// sbl_prim.h -- the rocPRIM device algorithms of the host code, each behind one call: ask for the temporary storage, grow the caller's
// DevBuf to it, run.  Every call site passes its own temporary buffer (nothing is shared between phases that was not shared before);
// functors and iterators (rocprim::plus, counting_iterator, ...) stay with the caller.  The *_bytes forms only ask: for a site that
// sizes ONE buffer for several algorithms before it launches any of them (an ensure() must not free a buffer under a kernel in flight).
#pragma once
#include <rocprim/rocprim.hpp>

#include "sbl_common.h"

namespace prim {

// significant bits of v (at least 1): the end bit of a radix sort over keys <= v
inline unsigned bits_of(unsigned long long v) { unsigned b = 1; while (b < 64 && (v >> b)) b++; return b; }

// f(storage, bytes) is the rocPRIM call with everything but its first two arguments bound
template <class F> inline size_t query(F f) { size_t bytes = 0; HIP_TRY(f(nullptr, bytes)); return bytes; }
template <class F> inline void run(DevBuf &tmp, F f) { size_t bytes = query(f); tmp.ensure(bytes); HIP_TRY(f(tmp.p, bytes)); }

template <class K, class V>
size_t sort_pairs_bytes(hipStream_t s, K *kin, K *kout, V *vin, V *vout, size_t n, unsigned begin_bit, unsigned end_bit)
{
	return query([&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, kin, kout, vin, vout, n, begin_bit, end_bit, s); });
}
template <class K, class V>
void sort_pairs(hipStream_t s, DevBuf &tmp, K *kin, K *kout, V *vin, V *vout, size_t n, unsigned begin_bit, unsigned end_bit)
{
	run(tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, kin, kout, vin, vout, n, begin_bit, end_bit, s); });
}
template <class K>
void sort_keys(hipStream_t s, DevBuf &tmp, K *kin, K *kout, size_t n, unsigned begin_bit, unsigned end_bit)
{
	run(tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_keys(t, b, kin, kout, n, begin_bit, end_bit, s); });
}
template <class In, class Out, class T, class Op>
void exclusive_scan(hipStream_t s, DevBuf &tmp, In in, Out out, T init, size_t n, Op op)
{
	run(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, in, out, init, n, op, s); });
}
template <class In, class Out, class Op>
size_t inclusive_scan_bytes(hipStream_t s, In in, Out out, size_t n, Op op)
{
	return query([&](void *t, size_t &b) { return rocprim::inclusive_scan(t, b, in, out, n, op, s); });
}
template <class In, class Out, class Op>
void inclusive_scan(hipStream_t s, DevBuf &tmp, In in, Out out, size_t n, Op op)
{
	run(tmp, [&](void *t, size_t &b) { return rocprim::inclusive_scan(t, b, in, out, n, op, s); });
}
// out = the in[i] with flags[i] set, in order; *count_out = how many (in may be any iterator)
template <class In, class Flags, class Out, class Count>
void select(hipStream_t s, DevBuf &tmp, In in, Flags flags, Out out, Count count_out, size_t n)
{
	run(tmp, [&](void *t, size_t &b) { return rocprim::select(t, b, in, flags, out, count_out, n, s); });
}
template <class KeysIn, class ValsIn, class KeysOut, class ValsOut, class Count, class Op, class Eq>
void reduce_by_key(hipStream_t s, DevBuf &tmp, KeysIn keys, ValsIn vals, size_t n, KeysOut unique_out, ValsOut aggregates_out, Count count_out, Op op, Eq eq)
{
	run(tmp, [&](void *t, size_t &b) { return rocprim::reduce_by_key(t, b, keys, vals, n, unique_out, aggregates_out, count_out, op, eq, s); });
}

}      // namespace prim
