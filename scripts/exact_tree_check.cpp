// The host side of option `exact` on its own, for a sanitizer build: exact_tree_mode and build_exact_tree (rm_scene_host.cpp)
// over the scenes of tests/test_exact_queries.py, with the invariants the device walk relies on checked for every tree.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -g \
//       -o exact_tree_check scripts/exact_tree_check.cpp cpu_raymarcher_amd/csrc/rm_scene_host.cpp && ./exact_tree_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../cpu_raymarcher_amd/csrc/rm_scene_host.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what, const char *scene) {
    if (!ok) {
        std::printf("FAILED %s: %s\n", scene, what);
        ++failures;
    }
}

// every object in exactly one leaf, every leaf inside the id list, every box inside its parent's, skip links forward
void check_tree(const rmh::HostScene &s, const rmh::ExactTree &t, const char *scene) {
    const size_t n = s.prim_lo.size() / 3;
    std::vector<int> seen(n, 0);
    int leaves = 0;
    for (size_t i = 0; i < t.nodes.size(); ++i) {
        const RmBvhNode &nd = t.nodes[i];
        expect(nd.skip > static_cast<int>(i) && nd.skip <= static_cast<int>(t.nodes.size()), "skip link", scene);
        if (nd.leaf < 0) {
            for (size_t c = i + 1; c < static_cast<size_t>(nd.skip); c = static_cast<size_t>(t.nodes[c].skip))
                for (int k = 0; k < 3; ++k) expect(t.nodes[c].lo[k] >= nd.lo[k] && t.nodes[c].hi[k] <= nd.hi[k], "child box inside parent", scene);
            continue;
        }
        ++leaves;
        const int first = nd.leaf >> 8, cnt = nd.leaf & 0xFF;
        expect(first >= 0 && static_cast<size_t>(first) + cnt <= t.ids.size(), "leaf range", scene);
        for (int k = 0; k < cnt && static_cast<size_t>(first) + k < t.ids.size(); ++k) {
            const int id = t.ids[first + k];
            expect(id >= 0 && static_cast<size_t>(id) < n, "id range", scene);
            if (id < 0 || static_cast<size_t>(id) >= n) continue;
            ++seen[id];
            for (int a = 0; a < 3; ++a) expect(s.prim_lo[3 * id + a] >= nd.lo[a] && s.prim_hi[3 * id + a] <= nd.hi[a], "object box inside leaf", scene);
        }
    }
    for (size_t i = 0; i < n; ++i) expect(seen[i] == 1, "object in exactly one leaf", scene);
    expect(leaves == t.leaves, "leaf count", scene);
}

void run(const rmh::HostScene &s, int want_mode, const char *scene) {
    const int mode = rmh::exact_tree_mode(s);
    expect(mode == want_mode, "mode", scene);
    if (mode != 2) return;
    rmh::ExactTree t;
    expect(rmh::build_exact_tree(s, t), "build", scene);
    check_tree(s, t, scene);
    std::printf("%-28s mode %d, %zu nodes, %d leaves, depth %d\n", scene, mode, t.nodes.size(), t.leaves, t.depth);
}

unsigned long long state = 0x5EED5EEDull;
double uniform() {  // splitmix64
    state += 0x9E3779B97F4A7C15ull;
    unsigned long long z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return static_cast<double>(z >> 11) * (1.0 / 9007199254740992.0);
}

}  // namespace

int main() {
    std::string err;
    for (int n : {0, 1, 2, 3, 40, 300, 10000}) {
        std::vector<float> c(3 * static_cast<size_t>(n));
        std::vector<double> r(n);
        for (int i = 0; i < n; ++i) {
            for (int k = 0; k < 3; ++k) c[3 * i + k] = static_cast<float>(-1.5 + 3.0 * uniform());
            r[i] = 0.01 + 0.03 * uniform();
        }
        for (int accel : {0, 1, 2}) {
            rmh::HostScene s;
            const std::string name = std::to_string(n) + " spheres, accel " + std::to_string(accel);
            expect(rmh::build_scene(s, c.data(), r.data(), n, accel, err), "build_scene", name.c_str());
            run(s, n == 0 ? 0 : (accel == 2 ? 1 : 2), name.c_str());
            if (n >= 3) {
                std::vector<double> neg(r);
                neg[2] = -0.05;
                expect(rmh::build_scene(s, c.data(), neg.data(), n, accel, err), "build_scene", name.c_str());
                run(s, 0, (name + ", a negative radius").c_str());
            }
        }
    }
    for (int preset : {3, 5, 7, 8, 9}) {  // the primitive presets (the Dense Grid as primitives too)
        std::vector<rmh::PrimDesc> prims;
        if (!rmh::preset_prims(preset, prims)) continue;
        for (int accel : {0, 1, 2}) {
            rmh::HostScene s;
            const std::string name = "preset " + std::to_string(preset) + " as primitives, accel " + std::to_string(accel);
            expect(rmh::build_scene_general(s, prims.data(), static_cast<int>(prims.size()), accel, err), "build_scene_general", name.c_str());
            run(s, accel == 2 ? 1 : 2, name.c_str());
            std::vector<rmh::PrimDesc> scaled(prims);
            rmh::scale_transform(scaled[0].m, 1.0, 2.0, 1.0);
            expect(rmh::build_scene_general(s, scaled.data(), static_cast<int>(scaled.size()), accel, err), "build_scene_general", name.c_str());
            run(s, 0, (name + ", one scaled").c_str());
        }
    }
    for (int preset : {10, 12}) {  // expression forests
        std::vector<rmh::NodeDesc> nodes;
        std::vector<int> roots;
        if (!rmh::preset_nodes(preset, nodes, roots)) continue;
        rmh::HostScene s;
        const std::string name = "preset " + std::to_string(preset) + " (forest)";
        expect(rmh::build_scene_nodes(s, nodes.data(), static_cast<int>(nodes.size()), roots.data(), static_cast<int>(roots.size()), 1, err), "build_scene_nodes",
               name.c_str());
        run(s, 0, name.c_str());
    }
    std::printf(failures ? "%d FAILURES\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
