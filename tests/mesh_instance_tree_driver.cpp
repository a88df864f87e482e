// mesh_instance_tree_driver.cpp -- the host builder of the instance tree (csrc/instance_tree.h) and the layout of a set that lies
// under one (instance_tree_layout in csrc/mesh_layout.h): plain C++, no HIP, compiled with the HOST compiler under AddressSanitizer
// + UBSan by tests/test_mesh_instance_tree_host.py.
//   For K in {1, 2, 3, 5, 64, 65, 200, 1000} and leaf_size in {1, 2, 4}, with random boxes and with K identical ones:
//   the layout   records | boxes | skip | first | count | order: each region at a multiple of 8, in that order, disjoint, at least as
//                large as its array, all inside `total`;
//   the build    into ONE block of exactly `total` bytes, as a set holds it: the topology once, then instance_tree_fit TWICE, the
//                second time over moved boxes -- which is what a move does.  A write outside a region's room is an ASan report;
//   the tree     after each build: every instance in exactly one leaf, a leaf's box the union of its instances' boxes, an inner
//                node's the union of its two children's, K identical boxes split down to leaf_size all the same.
// Prints one line of counts; exit code 0 = every check holds, otherwise the first that fails is named on stderr.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../blackhole_geodesic_calculator_amd/csrc/instance_tree.h"
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

static const size_t REC = 18;      // doubles per record: R, t, then the world box at 12

static unsigned long long rng_state = 0x2545F4914F6CDD1Dull;
static double uniform()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

// the records' world boxes: random ones about `shift`, or all the same
static void fill_boxes(double *rec, size_t K, bool identical, double shift)
{
    for (size_t j = 0; j < K; j++) {
        double *b = rec + j * REC + 12;
        for (int c = 0; c < 3; c++) {
            const double lo = identical ? shift + c : shift + 20.0 * uniform() - 10.0, ext = identical ? 1.0 : 0.1 + uniform();
            b[c] = lo;
            b[3 + c] = lo + ext;
        }
    }
}

static int check_tree(const double *rec, size_t K, int32_t leaf, const int32_t *skip, const int32_t *first, const int32_t *count, size_t nn,
                      const int32_t *order, const double *box)
{
    std::vector<int> seen(K, 0);
    size_t next = 0;
    for (size_t i = 0; i < nn; i++) {
        const double *b = box + i * 6;
        if (count[i] > 0) {
            CHECK(count[i] <= leaf && (size_t)first[i] == next && (size_t)skip[i] == i + 1);
            double u[6];
            for (int32_t k = 0; k < count[i]; k++) {
                const int32_t j = order[next + (size_t)k];
                CHECK(j >= 0 && (size_t)j < K);
                seen[(size_t)j]++;
                const double *w = rec + (size_t)j * REC + 12;
                for (int c = 0; c < 3; c++) {
                    u[c] = k ? std::min(u[c], w[c]) : w[c];
                    u[3 + c] = k ? std::max(u[3 + c], w[3 + c]) : w[3 + c];
                }
                if (k) CHECK(order[next + (size_t)k - 1] < j);      // (a leaf's slots in the caller's order)
            }
            CHECK(std::memcmp(u, b, sizeof(u)) == 0);
            next += (size_t)count[i];
        } else {
            CHECK(first[i] == -1 && i + 2 < nn);
            const size_t l = i + 1, r = (size_t)skip[l];
            CHECK(r < nn && skip[r] == skip[i]);
            for (int c = 0; c < 3; c++) {
                CHECK(b[c] == std::min(box[l * 6 + c], box[r * 6 + c]));
                CHECK(b[3 + c] == std::max(box[l * 6 + 3 + c], box[r * 6 + 3 + c]));
            }
        }
    }
    CHECK(next == K);
    for (size_t j = 0; j < K; j++) CHECK(seen[j] == 1);
    return 0;
}

static int check_set(size_t K, int32_t leaf, bool identical)
{
    std::vector<int32_t> skip, first, count;
    int32_t depth = 0;
    morton_topology(K, leaf, skip, first, count, depth);
    const size_t nn = skip.size();
    CHECK(nn == instance_tree_nodes(K, leaf) && nn <= 2 * K - 1);
    // K boxes -- identical ones too -- are split down to leaf_size: ceil(K / 2^depth) <= leaf_size < ceil(K / 2^(depth - 1))
    CHECK((K + ((size_t)1 << depth) - 1) >> depth <= (size_t)leaf);
    if (depth > 0) CHECK((K + ((size_t)1 << (depth - 1)) - 1) >> (depth - 1) > (size_t)leaf);
    const InstanceTreeLayout g = instance_tree_layout(K, REC, nn);
    const size_t off[7] = {g.records, g.node_box, g.node_skip, g.node_first, g.node_count, g.inst_order, g.total};
    const size_t want[6] = {K * REC * 8, nn * 48, nn * 4, nn * 4, nn * 4, K * 4};
    CHECK(off[0] == 0 && g.total % 8 == 0);
    for (int r = 0; r < 6; r++) {
        CHECK(off[r] % 8 == 0);
        CHECK(off[r + 1] >= off[r] + want[r] && off[r + 1] < off[r] + want[r] + 8);     // (in order, no overlap, packed)
    }
    // one block of exactly total bytes (malloc'ed storage: aligned for doubles), the topology once, two builds
    std::vector<char> block(g.total);
    char *b = block.data();
    std::memcpy(b + g.node_skip, skip.data(), nn * 4);
    std::memcpy(b + g.node_first, first.data(), nn * 4);
    std::memcpy(b + g.node_count, count.data(), nn * 4);
    double *rec = (double *)(b + g.records);
    for (int build = 0; build < 2; build++) {
        fill_boxes(rec, K, identical, build ? -3.5 : 2.0);
        instance_tree_fit(rec + 12, REC, K, (const int32_t *)(b + g.node_skip), (const int32_t *)(b + g.node_first),
                          (const int32_t *)(b + g.node_count), nn, (int32_t *)(b + g.inst_order), (double *)(b + g.node_box));
        CHECK(std::memcmp(b + g.node_skip, skip.data(), nn * 4) == 0 && std::memcmp(b + g.node_count, count.data(), nn * 4) == 0);
        if (check_tree(rec, K, leaf, (const int32_t *)(b + g.node_skip), (const int32_t *)(b + g.node_first),
                       (const int32_t *)(b + g.node_count), nn, (const int32_t *)(b + g.inst_order), (const double *)(b + g.node_box)))
            return 1;
    }
    return 0;
}

int main()
{
    int sets = 0;
    for (size_t K : {1, 2, 3, 5, 64, 65, 200, 1000})
        for (int32_t leaf : {1, 2, 4})
            for (bool identical : {false, true}) {
                if (check_set(K, leaf, identical)) return 1;
                sets++;
            }
    std::printf("sets %d checks %d\n", sets, n_check);
    return 0;
}
