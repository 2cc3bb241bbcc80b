// geo::Arena (vqvae_amd/csrc/geo_common.h) on its own, no device involved: test_arena_host.py builds this program with the
// host side under AddressSanitizer and UndefinedBehaviorSanitizer and runs it.  A layout function is measured, carved from a
// heap block of exactly the measured size and every byte of every buffer written (one byte past a buffer would be past the
// block for the last one, and into a neighbour's bytes checked below for the others); one byte fewer is refused with the
// need in `off`; the optional group (mark / rewind) is taken where it fits and leaves no trace where it does not.
#include <cstdlib>
#include <cstring>

#include "geo_common.h"

namespace geo {
void set_error(const char *, ...) {}
}  // namespace geo

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            return 1;                                                    \
        }                                                                \
    } while (0)

namespace {

constexpr size_t N = 37;      // odd on purpose: every buffer ends inside a 256-byte unit

struct Bufs {
    char *a;
    double *b;
    int32_t *none;            // zero elements
    uint16_t *c;
    float *opt_f;             // the optional group
    double *opt_d;
    bool with_opt;
};

void lay_out(geo::Arena &ar, Bufs &o) {
    ar.take(o.a, N);                  // 37 bytes   -> 256
    ar.take(o.b, N);                  // 296 bytes  -> 512
    ar.take(o.none, 0);               // nothing
    ar.take(o.c, 3 * N);              // 222 bytes  -> 256
}
constexpr size_t NEED = 1024;

void lay_out_with_optional(geo::Arena &ar, Bufs &o) {
    lay_out(ar, o);
    const size_t m = ar.mark();
    ar.take(o.opt_f, N);              // 148 bytes  -> 256
    ar.take(o.opt_d, 2 * N);          // 592 bytes  -> 768
    o.with_opt = ar.ok();
    if (!o.with_opt) {
        ar.rewind(m);
        o.opt_f = nullptr;
        o.opt_d = nullptr;
    }
}
constexpr size_t NEED_WITH_OPTIONAL = NEED + 1024;

// writes every byte of every buffer that was handed out, each with its own value, then reads them back
int fill_and_verify(const Bufs &o) {
    if (o.a) memset(o.a, 0x11, N);
    if (o.b) memset(o.b, 0x22, N * sizeof(double));
    if (o.c) memset(o.c, 0x33, 3 * N * sizeof(uint16_t));
    if (o.opt_f) memset(o.opt_f, 0x44, N * sizeof(float));
    if (o.opt_d) memset(o.opt_d, 0x55, 2 * N * sizeof(double));
    auto all = [](const void *p, int v, size_t bytes) {
        for (size_t i = 0; i < bytes; ++i)
            if (static_cast<const unsigned char *>(p)[i] != v) return false;
        return true;
    };
    CHECK(!o.a || all(o.a, 0x11, N));
    CHECK(!o.b || all(o.b, 0x22, N * sizeof(double)));
    CHECK(!o.c || all(o.c, 0x33, 3 * N * sizeof(uint16_t)));
    CHECK(!o.opt_f || all(o.opt_f, 0x44, N * sizeof(float)));
    CHECK(!o.opt_d || all(o.opt_d, 0x55, 2 * N * sizeof(double)));
    return 0;
}

// carves `lay` from a heap block of exactly `bytes` bytes
template <typename Lay>
int carve(Lay lay, size_t bytes, geo::Arena *ar_out, Bufs *o, char **block) {
    *block = static_cast<char *>(malloc(bytes));
    CHECK(*block);
    *ar_out = geo::Arena(*block, bytes);
    *o = Bufs{};
    lay(*ar_out, *o);
    return fill_and_verify(*o);
}

int run() {
    Bufs o{};
    char *block = nullptr;
    geo::Arena ar;

    // measuring: sizes only, no pointer
    lay_out(ar, o);
    CHECK(ar.ok() && ar.off == NEED);
    CHECK(!o.a && !o.b && !o.none && !o.c);
    geo::Arena measure_opt;
    lay_out_with_optional(measure_opt, o);
    CHECK(measure_opt.ok() && measure_opt.off == NEED_WITH_OPTIONAL && o.with_opt);

    // carving exactly the measured size
    if (carve(lay_out, NEED, &ar, &o, &block)) return 1;
    CHECK(ar.ok() && ar.off == NEED);
    CHECK(o.a == block && (char *)o.b == block + 256 && (char *)o.none == block + 768 && (char *)o.c == block + 768);
    free(block);

    // one byte fewer: refused, `off` is the need, what lies past the end is not handed out
    if (carve(lay_out, NEED - 1, &ar, &o, &block)) return 1;
    CHECK(!ar.ok() && ar.off == NEED);
    CHECK(o.a == block && (char *)o.b == block + 256 && !o.c);
    CHECK(ar.take<char>(1) == nullptr && ar.off == NEED + 256);       // and every take after it
    free(block);

    // the optional group: there when it fits ...
    if (carve(lay_out_with_optional, NEED_WITH_OPTIONAL, &ar, &o, &block)) return 1;
    CHECK(ar.ok() && ar.off == NEED_WITH_OPTIONAL && o.with_opt);
    CHECK((char *)o.opt_f == block + NEED && (char *)o.opt_d == block + NEED + 256);
    free(block);
    // ... one byte short of it, and with no room past the rest: the rest alone, `off` where it was
    for (size_t bytes : {NEED_WITH_OPTIONAL - 1, NEED}) {
        if (carve(lay_out_with_optional, bytes, &ar, &o, &block)) return 1;
        CHECK(ar.ok() && ar.off == NEED && !o.with_opt && !o.opt_f && !o.opt_d);
        CHECK(o.a == block && (char *)o.c == block + 768);
        free(block);
    }
    // ... and a workspace too small for the rest stays refused after the rewind
    if (carve(lay_out_with_optional, NEED - 1, &ar, &o, &block)) return 1;
    CHECK(!ar.ok() && ar.off == NEED && !o.with_opt && !o.c);
    free(block);
    return 0;
}

}  // namespace

int main() {
    if (run()) return 1;
    puts("arena_check: ok");
    return 0;
}
