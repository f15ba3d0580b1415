// Host check of csrc/blob.h: the declaring half of PsiBlob and bind(), against a malloc'ed base.  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/blob_host_check.hip -o blob_host_check
//   blob_host_check
//
// Every case is the sequence of buffers one constructor of the library declares, at the smallest shape its GPU test uses and once with
// every optional buffer absent: {bytes copied, bytes reserved, how it starts, null when empty, name}.  For each it checks, with offsets
// computed here by the rule itself (declaration order, next multiple of 256, nothing for a buffer that reserves nothing):
//   - every offset is a multiple of 256, the offsets ascend in declaration order and `size` is the padded sum;
//   - a buffer that reserves nothing has the offset of the buffer behind it;
//   - a reserve larger than the copy is kept, and the copy's size is what a name's capacity reports;
//   - bind() writes base + offset into every field and nothing else: each field is a heap cell of exactly one pointer, and the bytes each
//     buffer reserves are then written through its field, in a base of exactly `size` bytes — a pointer written beside a field, an offset
//     past the blob or two buffers that overlap are an address-sanitizer error or a mismatch of the pattern read back;
//   - a field declared "null when empty" stays null when nothing is copied into it, and every field is null after bind(nullptr);
//   - find() gives a name's buffer, and nothing for an absent name, a prefix of a name or a name with a suffix.
// Exit status 1 at the first failure.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include "../psi-release_amd/csrc/blob.h"

enum Start { HOST, DEVICE, ZERO, ONES, RAW };
struct Decl { size_t bytes, reserve; Start start; bool or_null; const char *name; };
struct Case { const char *who; std::vector<Decl> decls; long zero_from; };   // zero_from: the declaration zero_begin is set before, -1: never

static size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s: %s: ", c.who, #cond);                         \
            printf(__VA_ARGS__);                                             \
            printf("\n");                                                    \
            return false;                                                    \
        }                                                                    \
    } while (0)

static bool run(const Case &c)
{
    const size_t n = c.decls.size();
    std::vector<unsigned char **> field(n);                      // one heap cell of exactly one pointer per field
    static unsigned char poison;
    for (size_t i = 0; i < n; i++) { field[i] = (unsigned char **)malloc(sizeof(unsigned char *)); *field[i] = &poison; }
    PsiBlob T;
    const char src = 0;
    size_t zero_begin = PsiBlob::NO_ZERO;
    for (size_t i = 0; i < n; i++) {
        const Decl &d = c.decls[i];
        if ((long)i == c.zero_from) zero_begin = T.zero_begin = T.size;
        PsiBuf *b = nullptr;
        switch (d.start) {
        case HOST: b = &T.upload(*field[i], &src, d.bytes, d.reserve == d.bytes ? 0 : d.reserve); break;
        case DEVICE: b = &T.copy(*field[i], &src, d.bytes, d.reserve == d.bytes ? 0 : d.reserve); break;
        case ZERO: b = &T.zero(*field[i], d.bytes, d.name); break;
        case ONES: b = &T.ones(*field[i], d.bytes, d.name); break;
        case RAW: b = &T.raw(*field[i], d.reserve); break;
        }
        if (d.or_null) b->or_null();
    }
    CHECK(T.bufs.size() == n, "%zu buffers", T.bufs.size());
    // ---- the layout, against the rule restated here
    size_t want = 0;
    for (size_t i = 0; i < n; i++) {
        const Decl &d = c.decls[i];
        const PsiBuf &b = T.bufs[i];
        CHECK(b.off == want && b.off % 256 == 0, "buffer %zu at %zu, the rule says %zu", i, b.off, want);
        CHECK(b.reserved == d.reserve && b.bytes == (d.start == RAW ? 0 : d.bytes) && b.bytes <= b.reserved, "buffer %zu: %zu of %zu bytes", i, b.bytes, b.reserved);
        CHECK(b.field == (void *)field[i], "buffer %zu binds another field", i);
        CHECK(i == 0 || b.off >= T.bufs[i - 1].off + T.bufs[i - 1].reserved, "buffer %zu begins inside buffer %zu", i, i - 1);
        if (i + 1 < n && d.reserve == 0) CHECK(T.bufs[i + 1].off == b.off, "the empty buffer %zu does not share buffer %zu's offset", i, i + 1);
        const PsiBuf::Kind kind = d.start == HOST ? PsiBuf::HOST : d.start == DEVICE ? PsiBuf::DEVICE : d.start == RAW ? PsiBuf::NONE : PsiBuf::FILL;
        CHECK(b.kind == kind && b.fill == (d.start == ONES ? 0xff : 0), "buffer %zu starts as kind %d, fill %d", i, (int)b.kind, b.fill);
        CHECK((b.src != nullptr) == (d.start == HOST || d.start == DEVICE), "buffer %zu: source", i);
        want += pad256(d.reserve);
    }
    CHECK(T.size == want && T.size % 256 == 0, "size %zu, the padded sum is %zu", T.size, want);
    CHECK(T.zero_begin == zero_begin, "zero_begin %zu", T.zero_begin);
    // ---- bind: one pointer per field, every reserved byte inside the blob and in one buffer only
    unsigned char *base = (unsigned char *)malloc(T.size);
    T.bind((char *)base);
    for (size_t i = 0; i < n; i++) {
        const bool null = c.decls[i].or_null && !T.bufs[i].bytes;
        CHECK(*field[i] == (null ? nullptr : base + T.bufs[i].off), "field %zu after bind", i);
        if (!null) memset(*field[i], (int)(i + 1), T.bufs[i].reserved);
    }
    for (size_t i = 0; i < n; i++)
        for (size_t k = 0; k < T.bufs[i].reserved && *field[i]; k++)
            CHECK((*field[i])[k] == (unsigned char)(i + 1), "byte %zu of buffer %zu was written through another field", k, i);
    T.bind(nullptr);
    for (size_t i = 0; i < n; i++) CHECK(*field[i] == nullptr, "field %zu after bind(nullptr)", i);
    free(base);
    // ---- names
    size_t names = 0;
    for (size_t i = 0; i < n; i++) {
        const char *nm = c.decls[i].name;
        if (!nm) continue;
        names++;
        const PsiBuf *b = T.find(nm);
        CHECK(b == &T.bufs[i] && b->off == T.bufs[i].off && b->bytes == c.decls[i].bytes, "name %s", nm);
        const std::string s(nm);
        CHECK(!T.find((s + "x").c_str()) && !T.find(s.substr(0, s.size() - 1).c_str()) && !T.find(s.substr(1).c_str()), "a part of %s resolves", nm);
    }
    CHECK(!T.find("absent") && !T.find(""), "an absent name resolves");
    for (size_t i = 0; i < n; i++) free(field[i]);
    printf("%-44s %2zu buffers, %8zu bytes, %zu names\n", c.who, n, T.size, names);
    return true;
}

static Decl up(size_t bytes) { return {bytes, bytes, HOST, false, nullptr}; }
static Decl up(size_t bytes, size_t reserve, bool or_null) { return {bytes, reserve, HOST, or_null, nullptr}; }
static Decl dev(size_t bytes) { return {bytes, bytes, DEVICE, false, nullptr}; }
static Decl raw(size_t bytes) { return {0, bytes, RAW, false, nullptr}; }
static Decl zero(size_t bytes, const char *name = nullptr) { return {bytes, bytes, ZERO, false, name}; }
static Decl ones(size_t bytes, const char *name = nullptr) { return {bytes, bytes, ONES, false, name}; }

// psi_lbs_create: V vertices, J joints in one chain, NB betas; compressed: the model has the compressed skinning rows Wc / Wj
static Case lbs_case(const char *who, size_t V, size_t J, size_t NB, bool compressed)
{
    const size_t Kpad = pad256(NB + (J - 1) * 9), Vpad = pad256(V), Npad = 3 * Vpad, tile = Kpad * 32 + 1088, JP = 64, WNZ = 8;
    const size_t wc = compressed ? WNZ * Vpad * 4 : 0, wj = compressed ? WNZ / 4 * Vpad * 4 : 0, n_sub = J * (J + 1) / 2, chunk = (n_sub + JP - 1) / JP > 8 ? (n_sub + JP - 1) / JP : 8;
    size_t items = 0;
    for (size_t j = 0; j < J; j++) items += (J - j + chunk - 1) / chunk;
    return {who, {up(Npad / 32 * tile * 4), up(Kpad * Npad * 4), up(Npad * 4), up(JP * Vpad * 4), up(JP * Vpad * 4), up(J * 12), up(J * 3 * (NB ? NB : 1) * 4),
                  up(wc, wc + 4, true), up(wj, wj + 4, true), up(J * 4), up(J * 4), up((J + 1) * 4), up((J > 1 ? J - 1 : 1) * 4), up(6 * JP * 4), up(n_sub),
                  up(items * 4), up(J + 1)}, -1};
}

// psi_nn_index_create: m points in 8-point leaves under 256-byte nodes; the grid's cell starts and pair records, or neither
static Case nn_case(const char *who, size_t m, size_t nodes, size_t leaves, size_t cells)
{
    const size_t cs = cells ? (cells + 1) * 4 : 0, gp = cells ? ((m + 1) / 2 + 4) * 2 * 16 : 0;
    return {who, {up(nodes * 256), up(leaves * 8 * 16), up(m * 16), up(cs, cs, true), up(gp, gp + 64, false)}, -1};
}

// psi_surface_crossings_create: F faces in chunk order, their caller's indices, the parts of the faces and the P x P skip matrix (or
// neither: both fields null), the faces in the caller's order
static Case crossings_case(const char *who, size_t F, size_t P)
{
    return {who, {up(F * 12), up(F * 4), up(P ? F * 4 : 0, P ? F * 4 : 0, true), up(P * P, P * P, true), up(F * 12)}, -1};
}

int main()
{
    const size_t B = 2, n_c = 256, hint = B * n_c * 4;
    const std::vector<Case> cases = {
        lbs_case("psi_lbs_create V 500 J 55 NB 20", 500, 55, 20, true),
        lbs_case("psi_lbs_create, dense weights, no betas", 500, 55, 0, false),
        nn_case("psi_nn_index_create m 65", 65, 2, 9, 4 * 4 * 4),
        nn_case("psi_nn_index_create m 65, no grid", 65, 2, 9, 0),
        {"psi_mesh_sdf_create 2 triangles", {up(2 * 48), up(2 * 96), up((8 + 1) * 4), up(2 * 4)}, -1},
        {"psi_raster_mesh_create nv 4 nf 2, labels", {dev(4 * 12), dev(2 * 12), {4 * 4, 4 * 4, DEVICE, true, nullptr}, zero(4)}, -1},
        {"psi_raster_mesh_create nv 4 nf 2, no labels", {dev(4 * 12), dev(2 * 12), {0, 4 * 4, DEVICE, true, nullptr}, zero(4)}, -1},
        {"psi_raster_bodies_create V 5 F 2", {up(2 * 12), up((5 + 1) * 4), up(2 * 12)}, -1},
        {"psi_body_overlap_create F 352", {up(352 * 12)}, -1},
        crossings_case("psi_surface_crossings_create F 352, 2 parts", 352, 2),
        crossings_case("psi_surface_crossings_create F 352, no parts", 352, 0),
        // N = 64 points of d = 3, k = 2 centres, R = 1 restart: P = 1 update slice, NWA = 1 assign workgroup
        {"psi_kmeans_create N 64 d 3 k 2 R 1", {raw(64 * 3 * 4), dev(1 * 2 * 3 * 4), raw(4), raw(4), raw(4), raw(8), raw(8), raw(64 * 4), raw(2 * 3 * 8), raw(2 * 4), raw(8)}, -1},
        // S = 2 scenes of B = 2 bodies: KdDev is 88 bytes, PsiSdfGrid 40
        {"fit_build_scenes S 2 B 2", {up(2 * 88), up(2 * 40), zero(B * 4)}, -1},
        // the shape of fit_create's table: uploaded constants, then zero_begin, then named and unnamed fills, an empty buffer among them
        {"fit_create (constants | zero_begin | state)", {up(12), up(300), up(1024), zero(B * 75 * 4), zero(B * 75 * 4, "adam_m"), zero(B * 75 * 4, "adam_v"), zero(256),
                                                         zero(0), zero(B * 500 * 12, "verts"), ones(hint, "nn_hint"), zero(B * 4, "spb"), zero(1000)}, 3},
        {"every buffer empty but the last", {up(0), {0, 0, HOST, true, nullptr}, dev(0), zero(0), raw(0), up(1)}, -1},
    };
    for (const Case &c : cases)
        if (!run(c)) return 1;
    printf("all %zu blobs laid out as declared\n", cases.size());
    return 0;
}
