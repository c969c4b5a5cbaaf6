// The host side of the measures on its own, for a sanitizer build: rm_measure_world and the argument checks of the three
// entries on a host-only context (no device is touched).  The code under test is rm_api.cpp: it and this file are compiled
// with the sanitizers, the library's other objects are taken as `make` left them.  From cpu_raymarcher_amd/csrc, after make:
//
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Xarch_host -fsanitize=address,undefined"
//   hipcc $F -c -o san_api.o rm_api.cpp && hipcc $F -x hip -c -o san_check.o ../../scripts/measure_check.cpp
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o measure_check san_check.o san_api.o \
//       $(ls build/*.o | grep -v rm_api.o) -ldl && ./measure_check
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../include/rm_raymarch.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

rm_lattice lattice(int nu, int nv, int nw) {
    rm_lattice l;
    std::memset(&l, 0, sizeof l);
    l.du[0] = 0.25f;
    l.du[1] = 0.03125f;
    l.dv[0] = 0.0625f;
    l.dv[1] = -0.1875f;
    l.dw[1] = 0.125f;
    l.dw[2] = 0.3125f;
    l.nu = nu;
    l.nv = nv;
    l.nw = nw;
    return l;
}

}  // namespace

int main() {
    rm_ctx *ctx = nullptr;
    expect(rm_create(-1, &ctx) == RM_OK && ctx, "a host-only context");
    alignas(8) char buffer[64];
    void *p = buffer;

    // rm_measure_world: a full record, an empty one, the refusals
    rm_measure m;
    std::memset(&m, 0, sizeof m);
    m.n_points = 8;
    m.n_inside = 8;
    for (int c = 0; c < 3; ++c) {
        m.sum1[c] = 4;
        m.sum2[c] = 4;
        m.sum2[3 + c] = 2;
        m.lo[c] = 0;
        m.hi[c] = 1;
    }
    rm_lattice unit = lattice(2, 2, 2);
    std::memset(unit.du, 0, 36);
    unit.du[0] = unit.dv[1] = unit.dw[2] = 1.0f;
    struct rm_measure_world w;
    expect(rm_measure_world(&unit, &m, &w) == RM_OK, "rm_measure_world");
    expect(w.cell_volume == 1.0 && w.volume == 8.0 && w.centroid[0] == 0.5 && w.centroid[2] == 0.5, "a cube of eight cells");
    expect(std::fabs(w.second[0] - 8.0 * 4.0 / 12.0) < 1e-12 && w.second[3] == 0.0 && w.area_estimate == 0.0, "its second moments");
    const rm_lattice skew = lattice(9, 7, 5);
    expect(rm_measure_world(&skew, &m, &w) == RM_OK && w.cell_volume > 0.0, "a skewed lattice");
    std::memset(&m, 0, sizeof m);
    expect(rm_measure_world(&skew, &m, &w) == RM_OK && std::isnan(w.centroid[1]) && w.volume == 0.0 && w.second[4] == 0.0, "the empty record");
    expect(rm_measure_world(nullptr, &m, &w) == RM_E_INVALID && rm_measure_world(&skew, nullptr, &w) == RM_E_INVALID &&
               rm_measure_world(&skew, &m, nullptr) == RM_E_INVALID,
           "null arguments");

    // the device entries and the host entry: RM_E_INVALID ahead of the overflow refusal ahead of RM_E_NO_DEVICE
    const rm_lattice good = lattice(17, 17, 17), slice = lattice(17, 17, 1), huge = lattice(65535, 1025, 129);
    expect(rm_measure_field_device(ctx, &good, p, RM_MESH_F64, 0.0, p, nullptr) == RM_E_NO_DEVICE, "dense: no device");
    expect(rm_measure_field_device(ctx, &slice, p, RM_MESH_F32, 0.0, p, nullptr) == RM_E_NO_DEVICE, "dense: a slice is fine");
    expect(rm_measure_field_device(ctx, &good, nullptr, RM_MESH_F64, 0.0, p, nullptr) == RM_E_INVALID, "dense: null values");
    expect(rm_measure_field_device(ctx, &good, p, 7, 0.0, p, nullptr) == RM_E_INVALID, "dense: value_type");
    expect(rm_measure_field_device(ctx, &good, p, RM_MESH_F64, NAN, p, nullptr) == RM_E_INVALID, "dense: iso");
    expect(rm_measure_field_device(ctx, &good, buffer + 4, RM_MESH_F64, 0.0, p, nullptr) == RM_E_INVALID, "dense: alignment");
    expect(rm_measure_tiles_device(ctx, &good, p, p, 8, p, p, 0.0, p, nullptr) == RM_E_NO_DEVICE, "tiles: no device");
    expect(rm_measure_tiles_device(ctx, &good, p, p, 9, p, p, 0.0, p, nullptr) == RM_E_INVALID, "tiles: n_kept");
    expect(rm_measure_tiles_device(ctx, &slice, p, p, 0, p, p, 0.0, p, nullptr) == RM_E_INVALID, "tiles: a count below 2");
    expect(rm_measure_tiles_device(ctx, &good, p, p, 1, nullptr, p, 0.0, p, nullptr) == RM_E_INVALID, "tiles: null dist");
    expect(rm_measure_tiles_device(ctx, &huge, p, p, 1, p, p, 0.0, p, nullptr) == RM_E_UNSUPPORTED, "tiles: the overflow refusal");
    rm_measure out;
    rm_sparse_info info;
    expect(rm_scene_measure(ctx, &good, 0.0, 1.0, &out, &info) == RM_E_NO_DEVICE, "scene: no device");
    expect(rm_scene_measure(ctx, &good, 0.0, 0.0, &out, nullptr) == RM_E_INVALID, "scene: lipschitz");
    expect(rm_scene_measure(ctx, &good, 0.0, 1.0, nullptr, nullptr) == RM_E_INVALID, "scene: null measure");
    expect(rm_scene_measure(ctx, &huge, 0.0, 1.0, &out, nullptr) == RM_E_UNSUPPORTED, "scene: the overflow refusal");
    rm_destroy(ctx);
    std::printf(failures ? "%d failure(s)\n" : "measure_check: all passed\n", failures);
    return failures ? 1 : 0;
}
