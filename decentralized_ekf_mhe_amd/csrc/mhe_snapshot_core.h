// mhe_snapshot_core.h — snapshots of single instances of a direct handle (dekf_save_instances, dekf_load_instances).
//
// Everything an instance keeps is indexed by its own local clock (mhe_epoch_core.h, mhe_pause_core.h): the window records at its local
// step, the sample stack at its local pushes, the EKF history at its local count, the tags and the arrival cost computed ahead.  So an
// instance can leave its slot: its record is a copy of every persistent per-instance array together with the two local counters, and
// loading it is the resume of mhe_pause_core.h with the state coming out of the record: the epochs that make the stored local step
// and count the next ones (t0 = next_T - step, which is negative when an old robot loads into a young handle; c0 = ekf_count - count).
// No core changes, so a loaded instance computes, bit for bit, what its source goes on to compute from the same samples.
//
// The state map (StateMap) is the list of what the state is: one entry per array with its base pointer, elements per instance, element
// size and indexing kind.  It is built once, next to alloc_state (host_common.h: state_map), and the handle's optional stores are
// appended where they are allocated.  Entries are kept in the order of their tags, so two handles with the same stores have the same
// record layout whatever the order of the calls that allocated them.
//
// A blob is SnapHeader | n records in the order of idx.  A record is SnapBooks | every entry of the map in its order, each padded to a
// multiple of 8 bytes (the padding zeroed).  Record sizes (Go1, N = 20, ekf_history = 256): plain 81 808 bytes, smoothing 108 520, cross
// 121 480; Go1 with foot states (ns = 21), plain, 100 720.  The EKF history is 55 296 of each; the header is 832 bytes.
// The copy loops compile lane-sequentially like their neighbours (tests/hostsim/snapshot_hostsim.cpp); on the device a workgroup walks
// the map for one instance (kernels.hip: k_save_instances, k_load_instances).  The record side of every copy is contiguous: consecutive
// lanes move consecutive elements.  The state side is contiguous too for an instance-major array (base[b * count + i]) and strided by B
// for an element-major one (base[i * B + b]: the EKF state and its history).  Every offset is a size_t: a record is around 100 KB, and
// b * bytes leaves an int at a few thousand instances.
#pragma once
#include "cfg.h"
#include "mhe_pause_core.h"

namespace dekf {

enum SnapKind { SNAP_INSTANCE_MAJOR = 0, SNAP_ELEMENT_MAJOR = 1 };
// tags of the handle's optional stores (the arrays of DevState take 0, 1, ... in the order of state_map); all below 64
enum SnapTag { SNAP_TAG_COV = 48, SNAP_TAG_WIN_X, SNAP_TAG_WIN_COV, SNAP_TAG_WIN_T1, SNAP_TAG_CROSS, SNAP_TAG_INNOV_NU, SNAP_TAG_INNOV_S,
               SNAP_TAG_INNOV_NIS, SNAP_TAG_INNOV_NIS_LEG, SNAP_TAG_INNOV_LOGLIK, SNAP_TAG_GATED };

struct SnapEntry {
    void* base;
    int count;                  // elements per instance
    unsigned char esize, kind;  // 4 (int) or 8 (double); SnapKind
    short tag;
};

constexpr int DEKF_SNAP_MAX_ENTRIES = 62;
DEKF_HD size_t snap_pad8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

struct StateMap {
    SnapEntry e[DEKF_SNAP_MAX_ENTRIES];
    int n, B;
    // host: inserts the entry in front of the first one with a larger tag; false when the tag is there already or the map is full
    inline bool add(void* base, int count, int esize, int kind, int tag) {
        if (n >= DEKF_SNAP_MAX_ENTRIES || tag < 0 || tag >= 64) return false;
        int at = n;
        for (int k = 0; k < n; ++k) {
            if (e[k].tag == tag) return false;
            if (e[k].tag > tag) { at = k; break; }
        }
        for (int k = n; k > at; --k) e[k] = e[k - 1];
        e[at] = {base, count, (unsigned char)esize, (unsigned char)kind, (short)tag};
        ++n;
        return true;
    }
    // bytes per instance of the arrays the map covers, and of their image in a record (every entry padded)
    inline size_t covered_bytes() const {
        size_t t = 0;
        for (int k = 0; k < n; ++k) t += (size_t)e[k].count * e[k].esize;
        return t;
    }
    inline size_t padded_bytes() const {
        size_t t = 0;
        for (int k = 0; k < n; ++k) t += snap_pad8((size_t)e[k].count * e[k].esize);
        return t;
    }
    inline unsigned long long stores() const {
        unsigned long long t = 0;
        for (int k = 0; k < n; ++k) t |= 1ull << e[k].tag;
        return t;
    }
};

// The host-side books at the head of a record: the instance's NEXT local step (0: restarted and not yet initialised, local tick -1) and
// its local EKF count, reduced as a resume reduces it (reduced_count), and its noise fields (host_common.h: pack_noise)
constexpr int DEKF_SNAP_NOISE = 13 * 3 + 2 * DEKF_MAX_JOINTS + 3 * 4;
struct SnapBooks {
    int step, count;
    double noise[DEKF_SNAP_NOISE];
};
static_assert(sizeof(SnapBooks) % 8 == 0, "a record's arrays start at a multiple of 8 bytes");

// The fixed header of a blob.  Everything behind n and rec_bytes is the fingerprint: the stores of the map, the settings, and the
// handle's parameters with the noise fields and the padding zeroed (host_common.h: structure_of).  Filled after a memset, compared
// with memcmp.
constexpr unsigned long long DEKF_SNAP_MAGIC = 0x31504e53464b4544ull;  // "DEKFSNP1"
constexpr int DEKF_SNAP_VERSION = 1;
struct SnapHeader {
    unsigned long long magic;
    int version, n;
    unsigned long long rec_bytes;
    unsigned long long stores;
    int solver, smoother, cross, innov;
    double nis_leg_max;
    dekf_params structure;
};
DEKF_HD size_t snap_header_bytes() { return (sizeof(SnapHeader) + 63) & ~(size_t)63; }
inline size_t snap_record_bytes(const StateMap& m) { return sizeof(SnapBooks) + m.padded_bytes(); }

// ---- the device cores
// one array of instance b against its image in a record (rec: the image's first element)
template <class T, bool SAVE>
DEKF_FN void snap_copy_entry(const SnapEntry& m, size_t B, size_t b, T* rec) {
    const size_t n = (size_t)m.count;
    if (m.kind == SNAP_INSTANCE_MAJOR) {
        T* const a = (T*)m.base + b * n;
        for (size_t i = (size_t)DEKF_LANE(); i < n; i += (size_t)DEKF_NLANES()) {
            if (SAVE) rec[i] = a[i];
            else a[i] = rec[i];
        }
    } else {
        T* const a = (T*)m.base + b;
        for (size_t i = (size_t)DEKF_LANE(); i < n; i += (size_t)DEKF_NLANES()) {
            if (SAVE) rec[i] = a[i * B];
            else a[i * B] = rec[i];
        }
    }
}
// every array of instance b against the record `rec` (its first byte: the books).  Workgroup `chunk` of `nchunks` takes the entries
// chunk, chunk + nchunks, ...; saving, chunk 0 also writes the books
template <bool SAVE>
DEKF_FN void snapshot_instance(const StateMap& m, int b, unsigned char* rec, const SnapBooks* books, int chunk, int nchunks) {
    if (SAVE && chunk == 0) {
        const double* const src = (const double*)books;
        double* const dst = (double*)rec;
        for (size_t i = (size_t)DEKF_LANE(); i < sizeof(SnapBooks) / 8; i += (size_t)DEKF_NLANES()) dst[i] = src[i];
    }
    size_t off = sizeof(SnapBooks);
    for (int k = 0; k < m.n; ++k) {
        const SnapEntry& e = m.e[k];  // (uniform in the workgroup)
        if (k % nchunks == chunk) {
            if (e.esize == 8) snap_copy_entry<double, SAVE>(e, (size_t)m.B, (size_t)b, (double*)(rec + off));
            else {
                snap_copy_entry<int, SAVE>(e, (size_t)m.B, (size_t)b, (int*)(rec + off));
                // (the padding of an odd number of ints: a blob's bytes are a function of the state alone)
                if (SAVE && (e.count & 1) && DEKF_LANE() == 0) ((int*)(rec + off))[e.count] = 0;
            }
        }
        off += snap_pad8((size_t)e.count * e.esize);
    }
}

// ---- the host's arithmetic
// The books of instance b.  active, step, count, t0, c0 as set_active_instance takes them (mhe_pause_core.h), all null on a handle
// without epochs, whose instances all stand at the handle's own step and count.  An active instance: its current local step and count;
// a paused one: those it stands at; a restarted one that is not yet initialised: step 0 (t0 is next_T).
DEKF_HD void snapshot_books(int b, const int* active, const int* step, const int* count, const int* t0, const int* c0, int next_T,
                            int ekf_count, int H, int* out_step, int* out_count) {
    const bool epochs = active != nullptr;
    const bool runs = !epochs || active[b];
    *out_step = !epochs ? next_T : (runs ? next_T - t0[b] : step[b]);
    *out_count = reduced_count(!epochs ? ekf_count : (runs ? ekf_count - c0[b] : count[b]), H);
}
// what a record may hold: a step the handle's clock can express without reaching the sentinel, a reduced count
DEKF_HD bool snapshot_books_valid(int step, int count, int H) { return step >= 0 && step < DEKF_EPOCH_PAUSED && count >= 0 && count < 2 * H; }
// dekf_load_instances on instance b: it is active, on the epochs of a resume.  t0 is negative when step exceeds next_T: every use of
// an epoch is a difference T - t0 with T >= next_T, which then is the local step and stays below 2^31 as long as the instance's own
// clock does; c0 is above -2 H, as after a fold.
DEKF_HD void load_instance(int b, int step, int count, int* active, int* t0, int* c0, int next_T, int ekf_count, int H) {
    active[b] = 1;
    t0[b] = next_T - step;
    c0[b] = ekf_count - reduced_count(count, H);
}
// idx[n]: every entry inside 0 .. B - 1 and named once (seen: B zeroed chars of scratch)
inline bool snapshot_indices_valid(const int* idx, int n, int B, unsigned char* seen) {
    for (int i = 0; i < n; ++i) {
        if (idx[i] < 0 || idx[i] >= B || seen[idx[i]]) return false;
        seen[idx[i]] = 1;
    }
    return true;
}

}  // namespace dekf
