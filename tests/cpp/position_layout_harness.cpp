// Prints the layouts of synthesis_amd/csrc/position_layout.hpp for queries given on stdin, one per line:
//   dedup N TMP MIRROR      -> k0 k1 i0 i1 head scan start out.my out.op out.pi out.v out_num tmp c_my c_op flip expand dst rows total
//   reanalyse N TMP CHUNK   -> sel skip dst job_my job_op job_row moved done counts tmp results total
//   columns CAP GID 0       -> the byte offsets of my op gid pi v from the base (gid: -1 when the column is null), then those of
//                              columns_from(.., 7) from its own columns, then POS_ROW_BYTES POS_ROW_GID_BYTES
//   carve ROWS PI V         -> carve_columns' my op pi v and the carve's end, then which of columns_in's pointers are null (my op gid pi v)
// An absent section prints as -1.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../synthesis_amd/csrc/position_layout.hpp"

static long long show(size_t o) { return o == syn::ABSENT ? -1ll : (long long)o; }
static long long diff(const void* p, const void* base) { return p ? (long long)((uintptr_t)p - (uintptr_t)base) : -1ll; }

int main() {
    char what[32];
    unsigned long long a = 0, b = 0, c = 0;
    while (std::scanf("%31s %llu %llu %llu", what, &a, &b, &c) == 4) {
        if (!std::strcmp(what, "dedup")) {
            const syn::DedupLayout L = syn::dedup_layout((size_t)a, (size_t)b, c != 0);
            const size_t o[] = {L.k0, L.k1, L.i0, L.i1, L.head, L.scan, L.start, L.out.my, L.out.op, L.out.pi, L.out.v, L.out_num, L.tmp,
                                L.c_my, L.c_op, L.flip, L.expand, L.dst, L.rows, L.total};
            for (size_t x : o) std::printf("%lld ", show(x));
            std::printf("\n");
        } else if (!std::strcmp(what, "reanalyse")) {
            const syn::ReanalyseLayout L = syn::reanalyse_layout((size_t)a, (size_t)b, (size_t)c);
            const size_t o[] = {L.sel, L.skip, L.dst, L.job_my, L.job_op, L.job_row, L.moved, L.done, L.counts, L.tmp, L.results, L.total};
            for (size_t x : o) std::printf("%lld ", show(x));
            std::printf("\n");
        } else if (!std::strcmp(what, "columns")) {
            void* base = reinterpret_cast<void*>((uintptr_t)4096);
            const syn::PositionColumns s = syn::columns_at(base, (size_t)a, b != 0);
            const syn::PositionColumns t = syn::columns_from(s, 7);
            std::printf("%lld %lld %lld %lld %lld ", diff(s.my, base), diff(s.op, base), diff(s.gid, base), diff(s.pi, base), diff(s.v, base));
            std::printf("%lld %lld %lld %lld %lld ", diff(t.my, s.my), diff(t.op, s.op), s.gid ? diff(t.gid, s.gid) : (t.gid ? 0ll : -1ll),
                        diff(t.pi, s.pi), diff(t.v, s.v));
            std::printf("%zu %zu\n", syn::POS_ROW_BYTES, syn::POS_ROW_GID_BYTES);
        } else if (!std::strcmp(what, "carve")) {
            syn::Carve cv;
            const syn::ColumnOffsets o = syn::carve_columns(cv, (size_t)a, b != 0, c != 0);
            void* base = reinterpret_cast<void*>((uintptr_t)4096);
            const syn::PositionColumns s = syn::columns_in(base, o);
            std::printf("%lld %lld %lld %lld %zu %d %d %d %d %d\n", show(o.my), show(o.op), show(o.pi), show(o.v), cv.at, !s.my, !s.op, !s.gid,
                        !s.pi, !s.v);
        } else {
            std::fprintf(stderr, "unknown query %s\n", what);
            return 2;
        }
    }
    return 0;
}
