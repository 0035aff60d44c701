// TEST INFRASTRUCTURE ONLY.  pause_hostsim.cpp (unchanged) plus the lane-sequential build of the snapshot cores
// (decentralized_ekf_mhe_amd/csrc/mhe_snapshot_core.h): the state map of host_common.h walked by the copy loops the kernels run, and
// the host's books of a save and a load as dekf_capi.hip keeps them, through the same functions.  Built as libsnapshot_hostsim.so by
// tests/snapshot_lib.py.
#include "pause_hostsim.cpp"

#include "../../decentralized_ekf_mhe_amd/csrc/mhe_snapshot_core.h"

// The stores a direct handle allocates beside DevState, which the harness keeps as the caller's arrays (null: the variant has none).
// t1 is the cross variant's lag-one store; the smoothing variant's t1 is a scratch of every update here and is left out.
struct Stores {
    double *cov, *xw, *cw, *l1, *zn;
    int smoother, cross;
};

static StateMap map_of(Sim* h, const Stores& st) {
    StateMap m;
    state_map(h->c, h->s, m);
    const int N = h->c.N, n2 = h->c.ns * h->c.ns;
    if (st.cov) m.add(st.cov, n2, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_COV);
    if (st.xw) m.add(st.xw, N * h->c.ns, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_WIN_X);
    if (st.cw) m.add(st.cw, N * n2, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_WIN_COV);
    if (st.l1) m.add(st.l1, (N - 1) * n2, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_WIN_T1);
    if (st.zn) m.add(st.zn, N * n2, 8, SNAP_INSTANCE_MAJOR, SNAP_TAG_CROSS);
    return m;
}
static SnapHeader header_of(Sim* h, const dekf_params* p, const StateMap& m, const Stores& st, int n) {
    return snapshot_header(*p, m, n, 1, st.smoother != 0, st.cross != 0, false, 0.0);
}

extern "C" {
// out[0]: bytes per instance the state map covers; out[1]: what alloc_state allocates for a handle of B instances with one solver
// slab; out[2]: of that, the arrays the map leaves out by name; out[3]: entries of the map
void hs_snapshot_map_bytes(const dekf_params* p, int B, long long* out) {
    DevCfg c;
    out[0] = out[1] = out[2] = out[3] = -1;
    if (fill_cfg(*p, B, c)) return;
    DevState s;
    std::vector<void*> blocks;
    size_t total = 0;
    alloc_state(c, s, 1, [&](size_t bytes) { total += bytes; void* q = std::calloc(1, bytes ? bytes : 8); blocks.push_back(q); return q; });
    StateMap m;
    state_map(c, s, m);
    out[0] = (long long)m.covered_bytes();
    out[1] = (long long)total;
    out[2] = (long long)state_map_excluded_bytes(c, 1);
    out[3] = m.n;
    for (void* q : blocks) std::free(q);
}
long long hs_snapshot_header_bytes(void) { return (long long)snap_header_bytes(); }
long long hs_snapshot_books_bytes(void) { return (long long)sizeof(SnapBooks); }
long long hs_snapshot_record_bytes(void* hv, const Stores* st) { return (long long)snap_record_bytes(map_of((Sim*)hv, *st)); }

// dekf_save_instances between update(T0 - 1) and update(T0): 0, or 1 for what the C ABI refuses with DEKF_ERR_INVALID
int hs_save_instances(void* hv, void* ev, void* pv, const dekf_params* p, const Stores* st, const int* idx, int n, unsigned char* blob,
                      long long bytes) {
    Sim* h = (Sim*)hv;
    Epochs* ep = (Epochs*)ev;
    Pauses* pz = (Pauses*)pv;
    if (!idx || !blob || n <= 0) return 1;
    std::vector<unsigned char> seen((size_t)h->c.B, 0);
    if (!snapshot_indices_valid(idx, n, h->c.B, seen.data())) return 1;
    const StateMap m = map_of(h, *st);
    const size_t hb = snap_header_bytes(), rb = snap_record_bytes(m);
    if ((size_t)bytes < hb + (size_t)n * rb) return 1;
    const SnapHeader hd = header_of(h, p, m, *st, n);
    std::memset(blob, 0, hb);
    std::memcpy(blob, &hd, sizeof(hd));
    for (int i = 0; i < n; ++i) {
        SnapBooks bk;
        std::memset(&bk, 0, sizeof(bk));
        snapshot_books(idx[i], pz->active.data(), pz->step.data(), pz->count.data(), ep->t0.data(), ep->c0.data(), h->pushes, h->ekf_count,
                       h->c.ekf_hist, &bk.step, &bk.count);
        pack_noise(*p, bk.noise);
        for (int chunk = 0; chunk < 3; ++chunk) snapshot_instance<true>(m, idx[i], blob + hb + (size_t)i * rb, &bk, chunk, 3);
    }
    return 0;
}
// dekf_load_instances: 0, or 1 with nothing applied
int hs_load_instances(void* hv, void* ev, void* pv, const dekf_params* p, const Stores* st, const int* idx, int n, const unsigned char* blob,
                      long long bytes) {
    Sim* h = (Sim*)hv;
    Epochs* ep = (Epochs*)ev;
    Pauses* pz = (Pauses*)pv;
    if (!idx || !blob || n <= 0) return 1;
    std::vector<unsigned char> seen((size_t)h->c.B, 0);
    if (!snapshot_indices_valid(idx, n, h->c.B, seen.data())) return 1;
    const StateMap m = map_of(h, *st);
    const size_t hb = snap_header_bytes(), rb = snap_record_bytes(m);
    if ((size_t)bytes < hb + (size_t)n * rb) return 1;
    const SnapHeader want = header_of(h, p, m, *st, n);
    if (std::memcmp(blob, &want, sizeof(want)) != 0) return 1;
    double noise[DEKF_SNAP_NOISE];
    pack_noise(*p, noise);
    for (int i = 0; i < n; ++i) {
        SnapBooks bk;
        std::memcpy(&bk, blob + hb + (size_t)i * rb, sizeof(bk));
        if (!snapshot_books_valid(bk.step, bk.count, h->c.ekf_hist) || std::memcmp(noise, bk.noise, sizeof(noise)) != 0) return 1;
    }
    for (int i = 0; i < n; ++i) {
        SnapBooks bk;
        std::memcpy(&bk, blob + hb + (size_t)i * rb, sizeof(bk));
        snapshot_instance<false>(m, idx[i], const_cast<unsigned char*>(blob) + hb + (size_t)i * rb, nullptr, 0, 1);
        load_instance(idx[i], bk.step, bk.count, pz->active.data(), ep->t0.data(), ep->c0.data(), h->pushes, h->ekf_count, h->c.ekf_hist);
    }
    return 0;
}

// The host's arithmetic alone on one instance.  An active instance with epochs (t0, c0) of a handle at (next_T, count), history depth
// H, is saved: out[0] | out[1] the step and count of its books; the record is loaded into a handle at (next_T2, count2): out[2] | out[3]
// the epochs written; out[4]: whether the books are what a record may hold
void hs_snapshot_arith(int t0, int c0, int next_T, int count, int H, int next_T2, int count2, int* out) {
    int active = 1, step = 0, cnt = 0;
    snapshot_books(0, &active, &step, &cnt, &t0, &c0, next_T, count, H, &out[0], &out[1]);
    out[4] = snapshot_books_valid(out[0], out[1], H);
    int a2 = 0, t2 = 0, c2 = 0;
    load_instance(0, out[0], out[1], &a2, &t2, &c2, next_T2, count2, H);
    out[2] = t2;
    out[3] = c2;
}
}  // extern "C"
