// mesh_layout_driver.cpp -- where a mesh object's arrays lie in its device allocations (csrc/mesh_layout.h: plain C++, no HIP),
// compiled with the HOST compiler under AddressSanitizer + UBSan by tests/test_mesh_layout_host.py:
//   the image    for nt in {1, 2, 3, 63, 64, 65, 1000}, nn in {1, nt, 2 nt - 1}, n_inner in {0, nn / 2, nt - 1} where a tree can
//                have those counts, with and without normals: every region at a multiple of 8, the regions in the stated order and
//                disjoint, each at least as large as its array; without normals the normals region is empty and the next one
//                starts where it would have.  Every array is then written into one block of total bytes, first and last byte: a
//                region that reaches past the block is an ASan report.
//   the move     for cap in {nt, nt + 1, 4 nt}: each array of every such exact image fits inside the same region of the image by
//                capacity mesh_image(2 cap - 1, cap, cap), which is what lets a mesh move from one into the other region by region.
//   the pins     four exact images as numbers, from the arithmetic bhg_mesh_create did by hand before this header existed.
//   the scratch  the refit's scratch and the build's storage for cap in {1, 3, 1000}: regions in order and disjoint, the build's
//                record and sort storage at multiples of 256, room for cap keys, cap values and 3 cap indices.
// Prints one line of counts; exit code 0 = every check holds, otherwise the first that fails is named on stderr.
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../blackhole_geodesic_calculator_amd/csrc/mesh_layout.h"

using namespace bhg;

static int n_check = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        n_check++;                                                                               \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "check %d failed, line %d: %s\n", n_check, __LINE__, #cond);    \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

// the room region r has: up to the next region's start, or the image's end
static size_t room(const MeshImage &g, int r) { return (r + 1 < MESH_REGIONS ? g.off[r + 1] : g.total) - g.off[r]; }

// can a tree over nt triangles have nn nodes, ni of them inner?  (every inner node has at least two children, every leaf at least
// one triangle)
static bool legal(size_t nt, size_t nn, size_t ni) { return nn >= 1 && ni < nn && nn - ni <= nt && nn >= 2 * ni + 1 && (ni > 0 || nn == 1); }

static int check_image(size_t nn, size_t nt, size_t ni, bool normals)
{
    const MeshImage g = mesh_image(nn, nt, ni, normals);
    const size_t want[MESH_REGIONS] = {nn * 48, nt * 72, normals ? nt * 72 : 0, nn * 4, nn * 4, nn * 4, nt * 4, nt * 4, nt * 12, ni * 4};
    CHECK(g.off[0] == 0);
    for (int r = 0; r < MESH_REGIONS; r++) {
        CHECK(g.off[r] % 8 == 0);
        CHECK(g.bytes[r] == want[r]);
        CHECK(room(g, r) >= g.bytes[r] && room(g, r) < g.bytes[r] + 8);     // (which is: in order, no overlap, packed)
        CHECK(g.off[r] + g.bytes[r] <= g.total);
    }
    CHECK(g.total % 8 == 0);
    if (!normals) {
        const MeshImage w = mesh_image(nn, nt, ni, true);
        CHECK(room(g, MESH_NORMALS) == 0 && g.off[MESH_SKIP] == g.off[MESH_NORMALS] && g.off[MESH_NORMALS] == w.off[MESH_NORMALS]);
        for (int r = MESH_SKIP; r < MESH_REGIONS; r++) CHECK(w.off[r] - g.off[r] == nt * 72);
    }
    std::vector<char> block(g.total);
    for (int r = 0; r < MESH_REGIONS; r++)
        if (g.bytes[r]) block[g.off[r]] = block[g.off[r] + g.bytes[r] - 1] = 1;
    for (size_t cap : {nt, nt + 1, 4 * nt}) {
        const MeshImage c = mesh_image(2 * cap - 1, cap, cap, normals);
        for (int r = 0; r < MESH_REGIONS; r++) CHECK(g.bytes[r] <= room(c, r));
    }
    return 0;
}

static int check_pin(size_t nn, size_t nt, size_t ni, bool normals, const size_t (&off)[MESH_REGIONS], size_t total)
{
    const MeshImage g = mesh_image(nn, nt, ni, normals);
    for (int r = 0; r < MESH_REGIONS; r++) CHECK(g.off[r] == off[r]);
    CHECK(g.total == total);
    return 0;
}

int main()
{
    int images = 0;
    for (size_t nt : {1, 2, 3, 63, 64, 65, 1000})
        for (size_t nn : {size_t(1), nt, 2 * nt - 1})
            for (size_t ni : {size_t(0), nn / 2, nt - 1})
                for (bool normals : {false, true}) {
                    if (!legal(nt, nn, ni)) continue;
                    if (check_image(nn, nt, ni, normals)) return 1;
                    images++;
                }
    // The pins.  bhg_mesh_create laid its image out by hand until this header (csrc/bhgeo_capi.hip lines 1817-1821 of the commit
    // before it): sizes b_box = 48 nn, b_tri = 72 nt, b_nrm = b_tri or 0, b_node = round8(4 nn), b_idx = round8(4 nt),
    // b_sv = round8(12 nt), b_lv = round8(4 n_inner); offsets o_tri = b_box, o_nrm = o_tri + b_tri, o_skip = o_nrm + b_nrm,
    // o_first = o_skip + b_node, o_count = o_first + b_node, o_order = o_count + b_node, o_slot = o_order + b_idx,
    // o_sv = o_slot + b_idx, o_lv = o_sv + b_sv, total = o_lv + b_lv.  Worked by hand:
    //                                    box  tri  nrm  skip first count order slot  sv    lv
    if (check_pin(3, 2, 1, true, {0, 144, 288, 432, 448, 464, 480, 488, 496, 520}, 528)) return 1;       // 144 144 144 16 16 16 8 8 24 8
    if (check_pin(3, 2, 1, false, {0, 144, 288, 288, 304, 320, 336, 344, 352, 376}, 384)) return 1;      // 144 144   0 16 16 16 8 8 24 8
    if (check_pin(1, 1, 0, false, {0, 48, 120, 120, 128, 136, 144, 152, 160, 176}, 176)) return 1;       //  48  72   0  8  8  8 8 8 16 0
    if (check_pin(5, 5, 2, true, {0, 240, 600, 960, 984, 1008, 1032, 1056, 1080, 1144}, 1152)) return 1; // 240 360 360 24 24 24 24 24 64 8

    // the refit's scratch: summary | area | vertices | normals, and the build's storage
    for (size_t cap : {1, 3, 1000})
        for (bool normals : {false, true}) {
            const size_t nn = 2 * cap - 1, nv = cap + 2, summary = 72;
            const RefitLayout g = refit_layout(summary, nn, nv, normals);
            CHECK(g.summary == 0 && g.area >= g.summary + summary && g.vertices >= g.area + nn * 8 && g.normals >= g.vertices + nv * 24);
            CHECK(g.total >= g.normals + (normals ? nv * 24 : 0) && (normals || g.total == g.normals));
            CHECK(g.area % 8 == 0 && g.vertices % 8 == 0 && g.normals % 8 == 0);
            std::vector<char> block(g.total);
            block[g.summary] = block[g.area + nn * 8 - 1] = block[g.vertices + nv * 24 - 1] = 1;
            if (normals) block[g.normals + nv * 24 - 1] = 1;
        }
    for (size_t cap : {1, 3, 1000})
        for (size_t sort_bytes : {1, 256, 4097}) {
            const size_t record = 56;
            const BuildLayout g = build_layout(record, cap, sort_bytes);
            CHECK(g.record == 0 && g.record % 256 == 0 && g.sort % 256 == 0);
            CHECK(g.keys_in >= g.record + record && g.keys_in % 256 == 0);     // (the record has its 256-byte block to itself)
            CHECK(g.keys_out >= g.keys_in + cap * 8 && g.vals_in >= g.keys_out + cap * 8 && g.triangles >= g.vals_in + cap * 4);
            CHECK(g.sort >= g.triangles + cap * 12 && g.total >= g.sort + sort_bytes);
            CHECK(g.keys_out % 8 == 0 && g.vals_in % 8 == 0 && g.triangles % 8 == 0);
            std::vector<char> block(g.total);
            block[g.keys_in + cap * 8 - 1] = block[g.keys_out + cap * 8 - 1] = block[g.vals_in + cap * 4 - 1] = 1;
            block[g.triangles + cap * 12 - 1] = block[g.sort + sort_bytes - 1] = 1;
        }
    std::printf("images %d checks %d\n", images, n_check);
    return 0;
}
