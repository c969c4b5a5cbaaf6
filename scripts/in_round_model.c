/* CPU model of the in-round march steps of the v2 wave loop (rm_render_v2.hip, section M) on C3: the Dense Sphere Grid
 * under the golden camera at 3840 x 2160, BVH.  It traces rays with the project's own C oracle, splits every ray's
 * sequence of getDistance evaluations into rounds of the wave loop and in-round steps by section M's rules, and prints
 * what each rule for "the leaf set at the new point is the round's" costs: lane rounds per pixel, and per 64-pixel
 * batch the wave's rounds and in-round trips, with the reasons an in-round run ends.
 *
 *   build:  mkdir -p scripts/bin && gcc -O2 -std=c11 -ffp-contract=off -fno-fast-math -fexcess-precision=standard \
 *               -o scripts/bin/in_round_model scripts/in_round_model.c -lm      (from the repository's root)
 *   run:    scripts/bin/in_round_model            (a few seconds; no GPU)
 *
 * The model: lanes are grouped into 8 x 8 pixel batches; a wave's rounds are the maximum over its lanes, its in-round
 * trips in its r-th round the maximum over its lanes' r-th rounds.  Every sixth batch in both directions over the whole
 * frame: 3 600 batches.  Refill, the deferred normals (0.30 rounds per pixel) and the binary32 lower bound of the
 * runner-up (the exact runner-up is used) are not modelled.  "today" is the rule before round 8 (a ball around the
 * round's point); its three figures are to be held against scripts/counts.py on a -DRM_COUNTS build.
 *
 * Round 12, test (3): the last two rows bound the runner-up by its own (exact) distance at the new point and everything behind it
 * by the third-nearest distance less dd (option `runner_up`), and then let the run follow the runner-up when it becomes the nearer
 * one (the take-over: 0.14 fewer wave rounds per batch for 7.5 lane events that each need a second exact evaluation by the whole
 * wave -- not built).  Every accepted step's value is asserted to be the oracle's distance.  The play is per lane, as above: a
 * lockstep play of the wave (trips in which no lane commits) is not modelled. */
#include <stdio.h>

#include "../oracle/rm_oracle.c"

#define W_ 3840
#define H_ 2160
#define MAXL 64
#define MAXSTEP 100

typedef struct {
    double t, d, second, third, enter, exit_; /* second, third: the exact distances of the runner-up and of the nearest candidate behind it */
    float p[3];
    unsigned long long set; /* leaves whose box contains p */
    int k1, k2;
} Step;

static BBox leaf_box[MAXL];
static const BVHNode *leaf_node[MAXL];
static int n_leaf;
static BBox root_box;
static int G;                 /* cells per axis */
static float g_org[3], g_inv[3];
static double g_cell[3];

static void collect(const BVHNode *n) {
    if (!n->left && !n->right) {
        if (n_leaf >= MAXL) { fprintf(stderr, "more than %d leaves\n", MAXL); exit(1); }
        leaf_box[n_leaf] = n->bounds;
        leaf_node[n_leaf++] = n;
        return;
    }
    if (n->left) collect(n->left);
    if (n->right) collect(n->right);
}

/* rm_render_v2.hip box_margin */
static float margin(const BBox *b, const float *p) {
    float m = p[0] - b->min[0];
    for (int k = 0; k < 3; k++) {
        float a = p[k] - b->min[k], c = b->max[k] - p[k];
        if (a < m) m = a;
        if (c < m) m = c;
    }
    return m;
}

static void cell_of(const float *p, int *c, float *g) {
    for (int k = 0; k < 3; k++) {
        g[k] = (p[k] - g_org[k]) * g_inv[k];
        int i = (int)g[k];
        c[k] = i < 0 ? 0 : i > G - 1 ? G - 1 : i;
    }
}

/* build_point_query_grid's rule with the lists grown by `grow` (the product: 0.0100, and 0.0001 on top) */
static int listed(int leaf, const int *c, double grow) {
    for (int k = 0; k < 3; k++) {
        double a = ((double)leaf_box[leaf].min[k] - (grow + 0.0001) - (double)g_org[k]) * (double)g_inv[k] - 0.01;
        double b = ((double)leaf_box[leaf].max[k] + (grow + 0.0001) - (double)g_org[k]) * (double)g_inv[k] + 0.01;
        int c0 = (int)floor(a), c1 = (int)floor(b);
        c0 = c0 < 0 ? 0 : c0 > G - 1 ? G - 1 : c0;
        c1 = c1 < 0 ? 0 : c1 > G - 1 ? G - 1 : c1;
        if (c[k] < c0 || c[k] > c1) return 0;
    }
    return 1;
}

static int trace(const ro_scene *s, const float *o, const float *dir, Scratch *sc, Step *st) {
    int n = 0;
    double total = 0;
    AccelState as;
    if (!accel_start(s, o, dir, sc, &as)) return 0;
    for (int i = 0; i < 100; i++) {
        float p[3];
        vec3_scaleAndAdd(p, o, dir, total);
        double skip = accel_step(s, o, dir, total, sc, &as);
        if (skip == -1) break;
        if (skip > 0) {
            total += skip;
            if (total > MAX_DIST) break;
            continue;
        }
        Step *e = &st[n++];
        e->t = total;
        memcpy(e->p, p, sizeof p);
        e->enter = sc->intervals[as.curIdx].tEnter;
        e->exit_ = sc->intervals[as.curIdx].tExit;
        e->set = 0;
        e->k1 = e->k2 = -1;
        double best = 1e300, second = 1e300, third = 1e300;
        for (int l = 0; l < n_leaf; l++)
            if (margin(&leaf_box[l], p) >= 0.f) {
                e->set |= 1ull << l;
                for (int j = 0; j < leaf_node[l]->nprims; j++) {
                    int id = leaf_node[l]->prims[j];
                    double v = prim_sdf(&s->prims[id], p);
                    if (v < best) { third = second; second = best; e->k2 = e->k1; best = v; e->k1 = id; }
                    else if (v < second) { third = second; second = v; e->k2 = id; }
                    else if (v < third) third = v;
                }
            }
        uint32_t cnt = 0;
        double dist = scene_get_distance(s, p, &cnt, sc);
        e->d = dist;
        e->second = second;
        e->third = third;
        total += dist;
        if (dist < EPSILON) break;
        if (total > MAX_DIST) break;
    }
    return n;
}

/* Round 9: per axis the thresholds lo[k] and nextup(hi[k]) of every leaf box and the root (rm_scene_host.cpp build_step_box),
 * sorted and distinct: two points in one half-open cell [T_i, T_i+1) on all three axes have the same leaves.  The strict
 * form, for comparison: thresholds lo[k] and hi[k], cells open on both sides. */
static float thr[3][4 * MAXL + 4], thr_strict[3][4 * MAXL + 4];
static int n_thr[3], n_thr_strict[3];
static int cmp_float(const void *a, const void *b) { float x = *(const float *)a, y = *(const float *)b; return x < y ? -1 : x > y; }
static int sort_unique(float *v, int n) {
    qsort(v, (size_t)n, sizeof(float), cmp_float);
    int m = 0;
    for (int i = 0; i < n; i++)
        if (m == 0 || v[i] != v[m - 1]) v[m++] = v[i];
    return m;
}
static void build_thresholds(void) {
    for (int k = 0; k < 3; k++) {
        int n = 0, ns = 0;
        for (int l = -1; l < n_leaf; l++) {
            const BBox *b = l < 0 ? &root_box : &leaf_box[l];
            thr[k][n++] = b->min[k];
            thr[k][n++] = nextafterf(b->max[k], INFINITY);
            thr_strict[k][ns++] = b->min[k];
            thr_strict[k][ns++] = b->max[k];
        }
        n_thr[k] = sort_unique(thr[k], n);
        n_thr_strict[k] = sort_unique(thr_strict[k], ns);
    }
}
/* q and p in one cell of the thresholds on every axis? */
static int same_cell(const float *q, const float *p, int strict) {
    for (int k = 0; k < 3; k++) {
        const float *T = strict ? thr_strict[k] : thr[k];
        const int n = strict ? n_thr_strict[k] : n_thr[k];
        float lo = -INFINITY, hi = INFINITY;
        for (int i = 0; i < n; i++) {
            if (T[i] <= q[k]) lo = T[i];
            else { hi = T[i]; break; }
        }
        if (strict) {
            if (!(q[k] > lo && p[k] > lo && p[k] < hi)) return 0;
        } else if (!(p[k] >= lo && p[k] < hi)) return 0;
    }
    return 1;
}

/* Round 11: the half-open threshold cells as a table (rm_scene_host.cpp build_cell_tab).  Every cell has a key -- the leaves
 * that contain its representative point (its lower threshold on each axis, -inf for the first cell) and whether the root
 * does -- and a merged box: the cells are visited in index order, a cell without a box grows a block from itself one layer
 * at a time in the order -x, +x, -y, +y, -z, +z, again and again until no direction accepts a layer (every cell of the
 * layer has the starting cell's key), and the block becomes the box of every cell in it that has none yet. */
static int ct_dim[3], *ct_box; /* per cell: lo[3], hi[3] as cell indices, hi exclusive */
static unsigned long long *ct_key; /* the cell's leaves */
static unsigned char *ct_root;     /* whether the root box contains the cell */
static float ct_T(int k, int i) { return i <= 0 ? -INFINITY : i > n_thr[k] ? INFINITY : thr[k][i - 1]; } /* cell i is [T(i), T(i + 1)) */
static int ct_index(const int *c) { return (c[2] * ct_dim[1] + c[1]) * ct_dim[0] + c[0]; }
static void ct_cell(const float *p, int *c) {
    for (int k = 0; k < 3; k++) {
        int i = 0;
        while (i < n_thr[k] && thr[k][i] <= p[k]) i++;
        c[k] = i;
    }
}
static int ct_layer_ok(const int *lo, const int *hi, int axis, int at, unsigned long long key, int root) {
    int a[3] = {lo[0], lo[1], lo[2]}, b[3] = {hi[0], hi[1], hi[2]}, c[3];
    a[axis] = at;
    b[axis] = at + 1;
    for (c[2] = a[2]; c[2] < b[2]; c[2]++)
        for (c[1] = a[1]; c[1] < b[1]; c[1]++)
            for (c[0] = a[0]; c[0] < b[0]; c[0]++)
                if (ct_key[ct_index(c)] != key || ct_root[ct_index(c)] != root) return 0;
    return 1;
}
static void build_cell_table(int merge) {
    for (int k = 0; k < 3; k++) ct_dim[k] = n_thr[k] + 1;
    const int cells = ct_dim[0] * ct_dim[1] * ct_dim[2];
    ct_key = (unsigned long long *)calloc((size_t)cells, sizeof *ct_key);
    ct_root = (unsigned char *)calloc((size_t)cells, 1);
    ct_box = (int *)malloc((size_t)cells * 6 * sizeof(int));
    int c[3], in_root = 0, leafless = 0, most_leaves = 0, most_spheres = 0;
    for (c[2] = 0; c[2] < ct_dim[2]; c[2]++)
        for (c[1] = 0; c[1] < ct_dim[1]; c[1]++)
            for (c[0] = 0; c[0] < ct_dim[0]; c[0]++) {
                const float p[3] = {ct_T(0, c[0]), ct_T(1, c[1]), ct_T(2, c[2])};
                unsigned long long key = 0;
                int leaves = 0, spheres = 0;
                for (int l = 0; l < n_leaf; l++)
                    if (margin(&leaf_box[l], p) >= 0.f) {
                        key |= 1ull << l;
                        leaves++;
                        spheres += leaf_node[l]->nprims;
                    }
                const int root = margin(&root_box, p) >= 0.f;
                ct_root[ct_index(c)] = (unsigned char)root;
                in_root += root;
                leafless += root && leaves == 0;
                if (leaves > most_leaves) most_leaves = leaves;
                if (spheres > most_spheres) most_spheres = spheres;
                ct_key[ct_index(c)] = key;
                ct_box[6 * ct_index(c)] = -1;
            }
    int boxes = 0;
    for (c[2] = 0; c[2] < ct_dim[2]; c[2]++)
        for (c[1] = 0; c[1] < ct_dim[1]; c[1]++)
            for (c[0] = 0; c[0] < ct_dim[0]; c[0]++) {
                if (ct_box[6 * ct_index(c)] >= 0) continue;
                int lo[3] = {c[0], c[1], c[2]}, hi[3] = {c[0] + 1, c[1] + 1, c[2] + 1};
                const unsigned long long key = ct_key[ct_index(c)];
                const int root = ct_root[ct_index(c)];
                for (int grew = merge; grew;) {
                    grew = 0;
                    for (int axis = 0; axis < 3; axis++) {
                        if (lo[axis] > 0 && ct_layer_ok(lo, hi, axis, lo[axis] - 1, key, root)) { lo[axis]--; grew = 1; }
                        if (hi[axis] < ct_dim[axis] && ct_layer_ok(lo, hi, axis, hi[axis], key, root)) { hi[axis]++; grew = 1; }
                    }
                }
                boxes++;
                int d[3];
                for (d[2] = lo[2]; d[2] < hi[2]; d[2]++)
                    for (d[1] = lo[1]; d[1] < hi[1]; d[1]++)
                        for (d[0] = lo[0]; d[0] < hi[0]; d[0]++) {
                            int *b = ct_box + 6 * ct_index(d);
                            if (b[0] < 0) { memcpy(b, lo, sizeof lo); memcpy(b + 3, hi, sizeof hi); }
                        }
            }
    int sets = 0;
    for (int i = 0; i < cells; i++) {
        int seen = 0;
        for (int j = 0; j < i && !seen; j++) seen = ct_key[j] == ct_key[i];
        sets += !seen;
    }
    printf("cell table: %d x %d x %d = %d cells, %d in the root box of which %d without a leaf, %d distinct leaf sets, at most %d leaves "
           "and %d spheres per cell, %d merged boxes\n", ct_dim[0], ct_dim[1], ct_dim[2], cells, in_root, leafless, sets, most_leaves, most_spheres, boxes);
}
/* p in the merged box of q's cell? */
static int same_box(const float *q, const float *p) {
    int c[3];
    ct_cell(q, c);
    const int *b = ct_box + 6 * ct_index(c);
    for (int k = 0; k < 3; k++)
        if (!(p[k] >= ct_T(k, b[k]) && p[k] < ct_T(k, b[3 + k]))) return 0;
    return 1;
}

typedef struct {
    const char *name;
    int exact;      /* 0: the ball of rho and rho_cell; 1: the exact leaf set at p2; 2: one half-open threshold cell; 3: one open cell;
                     * 4: the merged box of q's threshold cell */
    double grow;    /* ball: how far the cell lists are grown */
    double confine; /* exact: p2 stays within q's cell grown by this; < 0: anywhere in the root box */
    int runner;     /* test (3), round 12 -- 0: every other candidate by second - dd; 1: the runner-up by its own distance at p2, the rest by
                     * third - dd (option `runner_up`); 2: ... and the run follows the runner-up when it becomes the nearer one (not built) */
} Rule;

enum { END_SET, END_CELL, END_INTERVAL, END_RUNNER, N_END };

static long takeovers, kept_by_runner;
/* may step j be taken in the round whose point is step h?  returns -1, or the reason it may not.  *win: the sphere the run follows
 * (h->k1 at its start; rule 2 may change it) */
static int refuse(const ro_scene *s, const Rule *r, const Step *h, const Step *e, int *win) {
    if (e->t < h->enter || e->t > h->exit_) return END_INTERVAL;
    float ex = e->p[0] - h->p[0], ey = e->p[1] - h->p[1], ez = e->p[2] - h->p[2];
    float dd = sqrtf(ex * ex + ey * ey + ez * ez) * 1.00001f + 1e-7f;
    int c[3];
    float g[3];
    cell_of(h->p, c, g);
    if (!r->exact) {
        float rho = margin(&root_box, h->p);
        for (int l = 0; l < n_leaf; l++)
            if (listed(l, c, r->grow)) {
                float m = fabsf(margin(&leaf_box[l], h->p));
                if (m < rho) rho = m;
            }
        double in_cell = 1e30;
        for (int k = 0; k < 3; k++) {
            double f = g[k] - (float)c[k];
            double v = (f < 1.0 - f ? f : 1.0 - f) * g_cell[k];
            if (v < in_cell) in_cell = v;
        }
        float rho_cell = (float)(r->grow + (in_cell > 0 ? in_cell : 0));
        if (!(dd < (rho < rho_cell ? rho : rho_cell))) return rho < rho_cell ? END_SET : END_CELL; /* whichever radius binds */
    } else if (r->exact >= 2) {
        if (r->exact == 4 ? !same_box(h->p, e->p) : !same_cell(h->p, e->p, r->exact == 3)) return END_SET;
        /* the rule's claim, checked against the oracle's sets on every accepted step */
        if (e->set != h->set || margin(&root_box, e->p) < 0.f) { fprintf(stderr, "threshold rule accepted a step whose leaf set differs\n"); exit(2); }
    } else {
        if (r->confine >= 0)
            for (int k = 0; k < 3; k++) {
                double lo = (double)g_org[k] + c[k] * g_cell[k] - r->confine, hi = (double)g_org[k] + (c[k] + 1) * g_cell[k] + r->confine;
                if (e->p[k] < lo || e->p[k] > hi) return END_CELL;
            }
        if (margin(&root_box, e->p) < 0.f || e->set != h->set) return END_SET;
    }
    double v = prim_sdf(&s->prims[*win], e->p);
    if (!((float)h->second - dd > (float)(v * (1 + 1e-6)))) {
        if (!r->runner || h->k2 < 0) return END_RUNNER;
        /* the other of the round's two nearest spheres by its own distance, everything behind them by third - dd */
        int other = *win == h->k1 ? h->k2 : h->k1;
        double w = prim_sdf(&s->prims[other], e->p);
        float rest = (float)h->third - dd;
        if ((float)(w * (1 - 1e-6)) > (float)(v * (1 + 1e-6)) && rest > (float)(v * (1 + 1e-6))) kept_by_runner += r->runner == 1;
        else if (r->runner == 2 && (float)(v * (1 - 1e-6)) > (float)(w * (1 + 1e-6)) && rest > (float)(w * (1 + 1e-6))) {
            *win = other; /* a second exact evaluation, by the whole wave, for this lane */
            v = w;
            takeovers += 1;
        } else return END_RUNNER;
    }
    /* the claim of test (3), on every accepted step: the value is the oracle's distance */
    if ((v < MAX_DIST ? v : MAX_DIST) != e->d) { fprintf(stderr, "rule '%s' accepted a step whose value is not the oracle's\n", r->name); exit(3); }
    return -1;
}

int main(void) {
    ro_scene *s = ro_scene_from_preset(3, "BVH");
    if (!s || !s->bvh) return 1;
    collect(s->bvh);
    root_box = s->bvh->bounds;
    build_thresholds();
    build_cell_table(1);
    G = (int)ceil(cbrt((double)n_leaf) * 3.0);
    G = G < 2 ? 2 : G > 32 ? 32 : G;
    for (int k = 0; k < 3; k++) {
        double ext = (double)root_box.max[k] - (double)root_box.min[k];
        g_org[k] = root_box.min[k];
        g_inv[k] = (float)(G / ext);
        g_cell[k] = 1.0 / (double)g_inv[k];
    }
    const Rule rules[] = {
        {"today: ball of rho, rho_cell", 0, 0.0100, 0},
        {"exact set, p2 in q's cell + 0.0100", 1, 0, 0.0100},
        {"exact set, p2 in q's cell + 0.24", 1, 0, 0.24},
        {"exact set, p2's own cell", 1, 0, -1},
        {"ball kept, lists grown by 0.06", 0, 0.06, 0},
        {"ball kept, lists grown by 0.24", 0, 0.24, 0},
        {"half-open threshold cells (round 9)", 2, 0, 0},
        {"open threshold cells", 3, 0, 0},
        {"merged threshold-cell boxes (round 11)", 4, 0, 0},
        {"... runner-up by its own distance (r12)", 4, 0, 0, 1},
        {"... and the run follows a take-over", 4, 0, 0, 2},
    };
    enum { NR = sizeof rules / sizeof rules[0] };
    double lane_rounds[NR] = {0}, lane_steps[NR] = {0}, wave_rounds[NR] = {0}, wave_trips[NR] = {0}, ends[NR][N_END] = {{0}};
    long batches = 0, pixels = 0;

    float rot[9];
    const float *ct = s->cameraTransform;
    rot[0] = ct[0]; rot[1] = ct[1]; rot[2] = ct[2]; rot[3] = ct[4]; rot[4] = ct[5]; rot[5] = ct[6]; rot[6] = ct[8]; rot[7] = ct[9]; rot[8] = ct[10];
    float org[3] = {ct[12], ct[13], ct[14]};
    Scratch sc;
    sc.cand = (int *)malloc((size_t)s->n * sizeof(int));
    sc.intervals = (Interval *)malloc((size_t)s->bvh_leaves * sizeof(Interval));
    sc.stack = (const BVHNode **)malloc((size_t)s->bvh_nodes * sizeof(BVHNode *));
    static Step st[MAXSTEP];
    static int trips[NR][64][MAXSTEP]; /* in-round trips of lane l's r-th round */
    static int rounds[NR][64];

    for (int by = 0; by < H_ / 8; by += 6)
        for (int bx = 0; bx < W_ / 8; bx += 6) {
            batches++;
            for (int l = 0; l < 64; l++) {
                int x = bx * 8 + (l & 7), y = by * 8 + (l >> 3);
                double u = ((double)x / W_ - 0.5) * 2.0, v = ((double)y / H_ - 0.5) * 2.0;
                float dir[3] = {f32(u), f32(v), -1.0f};
                vec3_transformMat3(dir, dir, rot);
                vec3_normalize(dir, dir);
                int n = trace(s, org, dir, &sc, st);
                pixels++;
                for (int r = 0; r < NR; r++) {
                    int nr = 0, h = 0, win = -1;
                    for (int j = 0; j < n; j++) {
                        int in_round = 0;
                        if (j > 0) {
                            const Step *q = &st[h];
                            /* aux.ok: leaves found, a winner, and no near tie with the runner-up */
                            int ok = q->set != 0 && q->k1 >= 0 && (float)q->second > (float)(q->d * (1 + 1e-6));
                            if (ok) {
                                int why = refuse(s, &rules[r], q, &st[j], &win);
                                if (why < 0) in_round = 1;
                                else ends[r][why] += 1;
                            }
                        }
                        if (in_round) {
                            trips[r][l][nr - 1]++;
                            lane_steps[r] += 1;
                        } else {
                            h = j;
                            win = st[j].k1;
                            trips[r][l][nr++] = 0;
                            lane_rounds[r] += 1;
                        }
                    }
                    rounds[r][l] = nr;
                }
            }
            for (int r = 0; r < NR; r++) {
                int wr = 0;
                for (int l = 0; l < 64; l++)
                    if (rounds[r][l] > wr) wr = rounds[r][l];
                wave_rounds[r] += wr;
                for (int k = 0; k < wr; k++) {
                    int m = 0;
                    for (int l = 0; l < 64; l++)
                        if (k < rounds[r][l] && trips[r][l][k] > m) m = trips[r][l][k];
                    wave_trips[r] += m;
                }
            }
        }
    printf("%d leaves, leaf grid %d^3, %ld batches of 64 pixels\n", n_leaf, G, batches);
    printf("%-38s %12s %12s %12s %12s   %s\n", "rule for continuing in M", "rounds/px", "steps/px", "wave rnd/b", "wave M/b", "run enders / px (set, cell, interval, runner-up)");
    for (int r = 0; r < NR; r++)
        printf("%-38s %12.2f %12.2f %12.2f %12.2f   %.2f / %.2f / %.2f / %.2f\n", rules[r].name, lane_rounds[r] / pixels, lane_steps[r] / pixels,
               wave_rounds[r] / batches, wave_trips[r] / batches, ends[r][END_SET] / pixels, ends[r][END_CELL] / pixels,
               ends[r][END_INTERVAL] / pixels, ends[r][END_RUNNER] / pixels);
    printf("runner-up by its own distance: %.2f lane steps per batch kept that second - dd refuses; take-over: %.2f lane take-overs per batch\n",
           (double)kept_by_runner / batches, (double)takeovers / batches);
    ro_scene_free(s);
    return 0;
}
