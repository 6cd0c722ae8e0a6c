// block.cpp — the libbsc block container and public C API on top of the GPU sorters and the host coder.
//
// Follows the container semantics of libbsc/libbsc/libbsc.cpp: bsc_store :68-81, bsc_compress :213-338
// (in-place twin :83-211), bsc_block_info :340-418, bsc_decompress :522-617; header layout
// [0]blockSize [4]dataSize [8]mode [12]index [16]adler(data) [20]adler(payload) [24]adler(header[0..24)),
// trailer = indexes[num] + num byte.  Stage entry points mirror bwt.cpp:178, st.cpp:990, coder.cpp:244.
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <mutex>
#include <condition_variable>
#include <deque>
#include <atomic>
#include <memory>
#include <thread>
#include <vector>
#include <algorithm>
#include <utility>

#include <sched.h>
#include <hip/hip_runtime.h>

#include "../../../include/libbsc.h"
#include "../../../include/bscgpu.h"
#include "../device/dev_common.h"
#include "../device/dma_copy.h"
#include "../device/dc_segment_plan.h"
#include "batch_pass_plan.h"
#include "container.h"
#include "qlfc.h"
#include "lzp.h"
#include "lzp_staged.h"
#include "par.h"

using namespace bschost;

// ---- allocator hooks (platform.cpp:173-190) ---------------------------------------------------------
static void* (*g_malloc)(size_t) = nullptr;
static void* (*g_zero_malloc)(size_t) = nullptr;
static void  (*g_free)(void*) = nullptr;
static void* bsc_malloc(size_t n) { return g_malloc ? g_malloc(n) : malloc(n); }
static void  bsc_free(void* p) { if (g_free) g_free(p); else free(p); }

// ---- process-wide default GPU contexts for the host-pointer API: one per visible device ----------------------------
// The reference keeps one cached arena behind one lock (bwt.cpp:50-52) and gets its parallelism from the CLI's OpenMP team
// calling bsc_compress concurrently, one block per thread (bsc.cpp:184-199).  Relinked against this library those calls
// are spread over ALL visible GPUs with no API change: every device has its own default contexts (two by default: their
// kernels interleave), GPU-stage locks and pinned slots.  Logical slot s lives on physical device s mod (number of devices), so
// the first context of every GPU comes before anybody's second one, and a call goes to the slot whose GPU has the fewest calls
// in flight (then the slot with the fewest; ties: round robin): N concurrent callers on an N-GPU node run one block per GPU, 2N
// callers two per GPU (bscgpu_dispatch_pick / bscgpu_dispatch_device below are that rule as pure functions, unit-tested on CPU).  BSC_GPU_DEVICE=<k> pins everything to device k; BSC_GPU_DEVICES=<n> uses the first n.
// The GPU stage of a call is serialised per device, but bsc_compress releases the lock before its host stage, so up to
// DEFAULT_SLOTS calls overlap per device — one on the GPU, the others coding on host threads.  A device's context is only
// re-created (for a larger block) when nobody is using it.
constexpr int       DEFAULT_SLOTS = 3;
constexpr int       MAX_DEVICES = 32;           // logical: contexts_per_device x physical devices
struct DefaultDevice {
    std::mutex   gpu_lock;                       // the GPU stage on this device
    bscgpu_ctx*  ctx = nullptr;
    int64_t      cap = 0;
    int          users = 0;
    bool         slot_busy[DEFAULT_SLOTS] = {false, false, false};
    int64_t      no_memory_for = -1;             // >= 0: creating this slot's context for a block this large failed for lack of HBM
};
static std::mutex   g_user_mu;                  // every DefaultDevice's ctx / cap / users / slot_busy, g_ndev, g_rr
static std::condition_variable g_user_cv;
static DefaultDevice g_dev[MAX_DEVICES];
static int          g_ndev = -1;                // logical devices the default path uses (-1: not probed yet)
static int          g_dev_first = 0;
static int          g_ctx_per_dev = 2;          // contexts per physical device: the kernels of two blocks interleave on the GPU and fill
                                                // the SIMDs that one block's serial chains leave idle (+14 % whole-job rate; BSC_GPU_CONTEXTS)
static unsigned     g_rr = 0;

// ---- the dispatch rule, as pure functions --------------------------------------------------------------------------
// Logical slots 0 .. nphys * ctx_per_dev - 1; slot s runs on physical device s % nphys.
extern "C" BSCGPU_API int bscgpu_dispatch_device(int slot, int nphys) { return nphys > 0 ? slot % nphys : 0; }
// users[s] = calls in flight on slot s; usable[s] != 0 when slot s can take this call now, 2 when its context already exists and is
// large enough (preferred among equally loaded slots: a lone caller then stays on one context instead of alternating between two and
// paying for two arenas, two sets of pinned buffers and every resize twice); start = round-robin cursor.
// Returns the slot to use, -1 when none is usable.
extern "C" BSCGPU_API int bscgpu_dispatch_pick(int nphys, int ctx_per_dev, const int* users, const unsigned char* usable, unsigned start)
{
    const int nslots = nphys * ctx_per_dev;
    if (nslots <= 0) return -1;
    int best = -1, best_dev_load = 0;
    for (int k = 0; k < nslots; ++k) {
        const int s = (int)((start + (unsigned)k) % (unsigned)nslots);
        if (!usable[s]) continue;
        int dev_load = 0;
        for (int q = s % nphys; q < nslots; q += nphys) dev_load += users[q];
        if (best < 0 || dev_load < best_dev_load ||
            (dev_load == best_dev_load && (users[s] < users[best] || (users[s] == users[best] && usable[s] > usable[best])))) { best = s; best_dev_load = dev_load; }
    }
    return best;
}

static int probe_devices_locked()
{
    if (g_ndev >= 0) return g_ndev;
    int n = bscgpu_device_count();
    if (n > MAX_DEVICES) n = MAX_DEVICES;
    g_dev_first = 0;
    if (const char* e = getenv("BSC_GPU_DEVICE")) { const int d = atoi(e); if (d >= 0 && d < n) { g_dev_first = d; n = 1; } else n = 0; }
    else if (const char* e2 = getenv("BSC_GPU_DEVICES")) { const int k = atoi(e2); if (k >= 1 && k < n) n = k; }
    if (const char* e3 = getenv("BSC_GPU_CONTEXTS")) { const int k = atoi(e3); if (k >= 1 && k <= 4) g_ctx_per_dev = k; }
    n *= g_ctx_per_dev;
    if (n > MAX_DEVICES) n = MAX_DEVICES / g_ctx_per_dev * g_ctx_per_dev;
    g_ndev = n;
    return n;
}

// Register as a user of a default context that can take n bytes; with want_slot also reserve a pinned slot.
static int default_gpu_acquire(int64_t n, bool want_slot, DefaultDevice** out, int* slot_out)
{
    std::unique_lock<std::mutex> lk(g_user_mu);
    const int ndev = probe_devices_locked();
    if (ndev <= 0) return LIBBSC_GPU_NOT_SUPPORTED;
    for (;;) {
        // the slot whose GPU is least loaded among those that can take the call right now (bscgpu_dispatch_pick)
        const int nphys = ndev / g_ctx_per_dev;
        int users[MAX_DEVICES]; unsigned char usable[MAX_DEVICES];
        bool any_ctx_fits = false;
        for (int d = 0; d < ndev; ++d) {
            DefaultDevice& D = g_dev[d];
            bool slot_free = !want_slot;
            for (int i = 0; i < DEFAULT_SLOTS && !slot_free; ++i) slot_free = !D.slot_busy[i];
            const bool fits = D.ctx && D.cap >= n;
            any_ctx_fits = any_ctx_fits || fits;
            users[d] = D.users;
            usable[d] = D.no_memory_for >= 0 && n >= D.no_memory_for ? 0 : (fits ? (slot_free ? 2 : 0) : (D.users == 0 ? 1 : 0));   // an idle slot can be (re)sized
        }
        const int best = bscgpu_dispatch_pick(nphys, g_ctx_per_dev, users, usable, g_rr);
        if (best >= 0) {
            DefaultDevice& D = g_dev[best];
            if (!(D.ctx && D.cap >= n)) {
                if (D.ctx) {
                    bscgpu_destroy(D.ctx); D.ctx = nullptr; D.cap = 0;
                    // HBM came back on this physical device: slots that had been taken out of the draw for lack of it are in again
                    for (int q = best % nphys; q < ndev; q += nphys) g_dev[q].no_memory_for = -1;
                }
                const int64_t cap = n + n / 32 + 4096;                    // headroom like bwt.cpp:106
                const int rc = bscgpu_create(&D.ctx, g_dev_first + bscgpu_dispatch_device(best, nphys), cap);
                if (rc != LIBBSC_NO_ERROR) {
                    D.ctx = nullptr;
                    // No HBM for one more arena of this size: if some other context can take the block, this slot is taken out
                    // of the draw for blocks this large and the caller queues for an existing context (large concurrent blocks
                    // queued before there were several contexts per GPU, too); otherwise the error is the caller's.
                    if (rc == LIBBSC_GPU_NOT_ENOUGH_MEMORY && any_ctx_fits) { D.no_memory_for = n; continue; }
                    return rc;
                }
                D.cap = cap;
                if (D.no_memory_for >= 0 && cap >= D.no_memory_for) D.no_memory_for = -1;     // it fits after all
            }
            int s = -1;
            if (want_slot) { for (int i = 0; i < DEFAULT_SLOTS; ++i) if (!D.slot_busy[i]) { s = i; break; } D.slot_busy[s] = true; }
            ++D.users;
            g_rr = (unsigned)best + 1u;
            *out = &D; if (slot_out) *slot_out = s;
            return LIBBSC_NO_ERROR;
        }
        // Nothing usable right now.  Somebody in flight will release a slot: wait.  Nobody in flight: nothing can change by itself — the
        // slots are all marked "no memory for this size" by an earlier failure — so the marks are dropped and creation is tried again
        // (the HBM may be free again: other processes, destroyed pipes); a second failure is the caller's error.
        bool in_flight = false, marked = false;
        for (int d = 0; d < ndev; ++d) { in_flight = in_flight || g_dev[d].users > 0; marked = marked || g_dev[d].no_memory_for >= 0; }
        if (!in_flight) {
            if (!marked) return LIBBSC_GPU_NOT_ENOUGH_MEMORY;
            for (int d = 0; d < ndev; ++d) g_dev[d].no_memory_for = -1;
            continue;
        }
        g_user_cv.wait(lk);
    }
}
static void default_gpu_release(DefaultDevice* D, int slot)
{
    { std::lock_guard<std::mutex> lk(g_user_mu); if (slot >= 0) D->slot_busy[slot] = false; --D->users; }
    g_user_cv.notify_all();
}
struct DefaultGpuUser {                         // RAII around acquire / release
    DefaultDevice* dev = nullptr; bscgpu_ctx* c = nullptr; int slot = -1; int rc;
    DefaultGpuUser(int64_t n, bool want_slot) { rc = default_gpu_acquire(n, want_slot, &dev, &slot); if (rc == LIBBSC_NO_ERROR) c = dev->ctx; }
    ~DefaultGpuUser() { if (rc == LIBBSC_NO_ERROR) default_gpu_release(dev, slot); }
};

extern "C" {

int bsc_init_full(int features, void* (*malloc_fn)(size_t), void* (*zero_malloc_fn)(size_t), void (*free_fn)(void*))
{
    (void)features;
    g_malloc = malloc_fn; g_zero_malloc = zero_malloc_fn; g_free = free_fn;
    (void)qlfc_tables();
    return LIBBSC_NO_ERROR;
}
int bsc_init(int features) { return bsc_init_full(features, nullptr, nullptr, nullptr); }
int bsc_bwt_init(int) { return LIBBSC_NO_ERROR; }
int bsc_st_init(int) { return LIBBSC_NO_ERROR; }
int bsc_coder_init(int) { (void)qlfc_tables(); return LIBBSC_NO_ERROR; }

unsigned int bsc_adler32(const unsigned char* T, int n, int) { return adler32(T, n < 0 ? 0 : (size_t)n); }

int bsc_coder_compress(const unsigned char* in, unsigned char* out, int n, int coder, int features)
{ return coder_compress(in, out, n, coder, features); }
int bsc_coder_decompress(const unsigned char* in, unsigned char* out, int coder, int features)
{ return coder_decompress(in, out, coder, features); }
int bsc_qlfc_encode_block(const unsigned char* in, unsigned char* out, int inSize, int outSize, int coder)
{ return qlfc_encode_block(in, out, inSize, outSize, coder); }
int bsc_qlfc_decode_block(const unsigned char* in, unsigned char* out, int coder)
{ return qlfc_decode_block(in, out, coder); }
int bsc_qlfc_ranks(const unsigned char* in, int n, unsigned char* ranks, unsigned char* firstSeen, int* pK)
{
    QlfcRuns R;
    qlfc_runs(in, n, R);
    memcpy(ranks, R.rank.data(), R.rank.size());
    memcpy(firstSeen, R.view.first_seen, (size_t)R.view.nsym);
    if (pK) *pK = R.view.nsym;
    return (int)R.rank.size();
}

// ---- sorters: GPU only ---------------------------------------------------------------------------------
int bsc_bwt_encode(unsigned char* T, int n, unsigned char* num_indexes, int* indexes, int features)
{
    (void)features;
    if (T == nullptr || n < 0) return LIBBSC_BAD_PARAMETER;
    // n = 0: the reference hands libsais an empty text; with the secondary indexes asked for, r = 1 is rejected first (libsais.c:6711)
    if (n == 0) return (num_indexes != nullptr && indexes != nullptr) ? LIBBSC_BAD_PARAMETER : 0;
    if (num_indexes != nullptr && indexes != nullptr && aux_rate(n) < 2) return LIBBSC_BAD_PARAMETER;     // (no GPU needed to say so)
    DefaultGpuUser user(n, false);
    if (user.rc != LIBBSC_NO_ERROR) return user.rc;
    bscgpu_ctx* c = user.c;
    std::lock_guard<std::mutex> g(user.dev->gpu_lock);
    if (num_indexes != nullptr && indexes != nullptr) {
        const int r = aux_rate(n);
        if (r < 2) return LIBBSC_BAD_PARAMETER;               // libsais_bwt_aux rejects r < 2 (libsais.c:6711)
        uint32_t I[256];
        const int cnt = (n - 1) / r;
        if (cnt + 1 > 256) return LIBBSC_BAD_PARAMETER;
        int64_t res = bscgpu_bwt_aux(c, T, T, n, r, I);
        if (res < 0) return (int)res;
        *num_indexes = (unsigned char)cnt;
        for (int t = 0; t < cnt; ++t) indexes[t] = (int)I[t + 1] - 1;     // bwt.cpp:205-209
        return (int)I[0];
    }
    return (int)bscgpu_bwt(c, T, T, n);
}

// inverse BWT on the default GPU context (decode.cpp calls this for large blocks; < 0 other than DATA_CORRUPT = not available,
// the caller continues on the host)
int bsc_bwt_decode_gpu(unsigned char* T, int n, int index)
{
    DefaultGpuUser user(n, false);
    if (user.rc != LIBBSC_NO_ERROR) return user.rc;
    std::lock_guard<std::mutex> g(user.dev->gpu_lock);
    return bscgpu_unbwt(user.c, T, T, n, index);
}

int bsc_st_encode(unsigned char* T, int n, int k, int features)
{
    (void)features;
    if (T == nullptr || n < 0) return LIBBSC_BAD_PARAMETER;
    if (k < 3 || k > 8) return LIBBSC_BAD_PARAMETER;
    if (n <= 1) return 0;
    DefaultGpuUser user(n, false);
    if (user.rc != LIBBSC_NO_ERROR) return user.rc;
    std::lock_guard<std::mutex> g(user.dev->gpu_lock);
    return bscgpu_st_encode(user.c, T, n, k);
}

// ---- container ---------------------------------------------------------------------------------------------
int bsc_store(const unsigned char* input, unsigned char* output, int n, int)
{
    const unsigned a = adler32(input, (size_t)n);
    memmove(block_body(output), input, (size_t)n);
    return block_finish_stored(output, n, a);
}

// the stored rule (libbsc.cpp:188) for a block whose input is in HBM: one copy of it straight into the output region
static int store_from_device(bscgpu_ctx* c, const void* dIn, unsigned char* output, int n, unsigned adler)
{
    if (hipSetDevice(c->device) != hipSuccess || hipMemcpy(block_body(output), dIn, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
        return LIBBSC_GPU_ERROR;
    return block_finish_stored(output, n, adler);
}

static int make_mode(int sorter, int coder, int lzpHashSize, int lzpMinLen, int* mode_out)
{
    if (sorter != LIBBSC_BLOCKSORTER_BWT && (sorter < LIBBSC_BLOCKSORTER_ST3 || sorter > LIBBSC_BLOCKSORTER_ST8)) return LIBBSC_BAD_PARAMETER;
    if (coder < LIBBSC_CODER_QLFC_STATIC || coder > LIBBSC_CODER_QLFC_FAST) return LIBBSC_BAD_PARAMETER;
    if (lzpMinLen != 0 || lzpHashSize != 0) {
        if (lzpMinLen < 4 || lzpMinLen > 255) return LIBBSC_BAD_PARAMETER;
        if (lzpHashSize < 10 || lzpHashSize > 28) return LIBBSC_BAD_PARAMETER;
    }
    *mode_out = block_mode_pack(BlockMode{sorter, coder, lzpHashSize, lzpMinLen});
    return LIBBSC_NO_ERROR;
}

int bsc_block_info(const unsigned char* hdr, int headerSize, int* pBlockSize, int* pDataSize, int)
{
    if (headerSize < LIBBSC_HEADER_SIZE) return LIBBSC_UNEXPECTED_EOB;
    BlockFields h;
    if (!block_header_read(hdr, &h)) return LIBBSC_DATA_CORRUPT;
    const int blockSize = h.block_size, dataSize = h.data_size, index = h.index;
    const BlockMode m = block_mode_unpack(h.mode);

    // every field a value the format knows (0: a stored block has neither sorter nor coder), and no bit of the mode word outside them
    if (m.sorter != 0 && m.sorter != LIBBSC_BLOCKSORTER_BWT && (m.sorter < LIBBSC_BLOCKSORTER_ST3 || m.sorter > LIBBSC_BLOCKSORTER_ST8)) return LIBBSC_DATA_CORRUPT;
    if (m.coder != 0 && (m.coder < LIBBSC_CODER_QLFC_STATIC || m.coder > LIBBSC_CODER_QLFC_FAST)) return LIBBSC_DATA_CORRUPT;
    if (m.lzp_min != 0 || m.lzp_hash != 0) {
        if (m.lzp_min < 4 || m.lzp_min > 255) return LIBBSC_DATA_CORRUPT;
        if (m.lzp_hash < 10 || m.lzp_hash > 28) return LIBBSC_DATA_CORRUPT;
    }
    if (block_mode_pack(m) != h.mode) return LIBBSC_DATA_CORRUPT;
    if (blockSize < LIBBSC_HEADER_SIZE || blockSize > LIBBSC_HEADER_SIZE + dataSize) return LIBBSC_DATA_CORRUPT;
    if (index < 0 || index > dataSize) return LIBBSC_DATA_CORRUPT;
    if (pBlockSize) *pBlockSize = blockSize;
    if (pDataSize) *pDataSize = dataSize;
    return LIBBSC_NO_ERROR;
}

// ---- GPU-resident compress: Adler-32 + sorter + QLFC front end on the device, QLFC coding on host threads ----
// One block = a GPU stage (runs on the submitting thread, serialised per context) and a host stage (worker thread).
struct BlockJob {
    bscgpu_ctx* c = nullptr;
    const void* dInput = nullptr;
    const uint8_t* hInput = nullptr; // host copy of the original block (bsc_compress); null for device-resident callers
    uint8_t*    output = nullptr;
    int n_orig = 0;                  // size of the original block; n below is what the sorter sees (LZP output or the same)
    bool have_adler = false, inplace = false;
    std::unique_ptr<unsigned char, void (*)(void*)> lz{nullptr, nullptr};   // LZP output while the block is in flight
    // BSCGPU_OPT_DEVICE_LZP: the block goes up raw and the device stage (lzp.hip) writes the sorter's input; lz is not made
    bool dev_lzp = false; int lzp_hash = 0, lzp_min = 0, mode_with_lzp = 0;
    const void* dRaw = nullptr;      // ... the raw block in HBM where the caller's input is there (bscgpu_compress_device_lzp); null: it is uploaded from hInput
    int n = 0, coder = 0, features = 0, mode = 0, index = 0, num_indexes = 0, nblocks = 0;
    int indexes[256];
    uint32_t adler_data = 0;
    int start[8], size[8];
    u32 run_first[9];
    u32 first_run[8 * 256];
    HostSlot* slot = nullptr;        // pinned landing zones of this block (owned by the context)
    // device-side static model (devcoder.hip): the host codes from a probability stream instead of run arrays
    bool pipelined = false;        // submitted through a pipe (several blocks in flight): throughput over latency
    int  pipe_workers = 0;         // coder threads of the process-wide pool (0: a synchronous call, which starts its own threads)
    int  pool_free = -1;           // CPUs of the pool's budget with nothing to do when the block was queued (-1: not a pipe's block)
    int  tail_r = -1;              // blocks of the announced job whose GPU stage was still to END when this one's did (-1: no job announced)
    int  tail_gpus = 1;            // ... and how many GPUs feed the pool in that job
    int  tail_pipes = 6;           // ... and how many pipes (GPU contexts) per GPU: that many blocks' GPU stages overlap
    int  ps_g = 2;                 // device-model sub-blocks per coder task (ps_group), fixed when the block's host work starts
    bool use_ps = false; const uint16_t* ps = nullptr; u32 poff[9]; u32 ndec = 0; int sorter = 0;
    bool ps_packed = false; u32 pbase[9];          // the stream is the 13-bit packed form (devcoder.hip DcP13): sub-block b's starts at decision pbase[b] of the packed space (a multiple of 64)
    // sub-block b's stream as the coders take it: 16-bit entries, or the packed bytes
    const void* ps_of(int b) const { return ps_packed ? static_cast<const void*>(reinterpret_cast<const uint8_t*>(ps) + (size_t)pbase[b] / 8u * 13u) : ps + poff[b]; }
    hipEvent_t ps_ready = nullptr;   // the p stream's copy to the host (copy stream), all of it
    hipEvent_t ps_part[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // ... up to and including sub-block b: what a coder task waits on
    bool ps_dma = false; uint64_t ps_sig[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the pieces went through the DMA engine directly (dma_copy.h): signals instead of events
    bool rc_done = false;            // BSCGPU_OPT_DEVICE_RC: the GPU stage has range-coded the sub-blocks as well (scratch / sub_res are final, nothing crossed PCIe but them)
    // (a signal of 0: the piece was put into the landing zone by the host itself — a void segment of a block in sub-block segments)
    bool ps_landed(int b) const { return ps_dma ? ps_sig[b] == 0 || dma_wait(ps_sig[b]) == 0 : hipEventSynchronize(ps_part[b]) == hipSuccess; }
    std::atomic<bool> redo{false};   // a sub-block did not compress: the block goes through the host model again (raw sub-blocks need the run arrays)
    bool stored_small = false;       // n <= header size: finished in the GPU stage
    int  result = 0;
    // host stage, split into per-sub-block tasks for the pipe's worker pool
    RunView views[8];
    std::unique_ptr<uint8_t[]> scratch[8];          // coded sub-blocks; kept across the blocks of a pipe lane (no re-faulting)
    size_t scratch_cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int  sub_res[8];
    std::atomic<int> remaining{0};
    bool done = false;
};

using clk = std::chrono::steady_clock;
static double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

// BSC_DEVICE_CODER=0 keeps the static coder's model on the host; BSC_DEVICE_CODER_MIN_N: smallest block that takes the device model
static bool devcoder_enabled() { static const int v = [] { const char* e = getenv("BSC_DEVICE_CODER"); return e ? atoi(e) : 1; }(); return v != 0; }
static int  devcoder_min_n() { static const int v = [] { const char* e = getenv("BSC_DEVICE_CODER_MIN_N"); return e ? atoi(e) : (1 << 20); }(); return v; }

static std::atomic<uint64_t> g_count_devmodel{0}, g_count_redo{0}, g_count_devmodel_lzp{0}, g_count_device_lzp{0};     // bscgpu_process_counter

// the entry form of a device-model block's probability stream (include/bscgpu.h)
static int ps_form(const BlockJob& J) { return J.ps_packed ? BSCGPU_RC_STATIC13 : J.coder == LIBBSC_CODER_QLFC_FAST ? BSCGPU_RC_FAST16 : BSCGPU_RC_STATIC16; }
// sub-block q's buffer for its coded bytes
static void sub_scratch(BlockJob& J, int q)
{
    const size_t need = (size_t)J.size[q] + 64;
    if (J.scratch_cap[q] < need) { J.scratch[q].reset(new uint8_t[need + need / 8]); J.scratch_cap[q] = need + need / 8; }
}
// sub-block q of a device-model block as the stream coders take it (qlfc.h); parallel framing semantics (coder.cpp:159-240): every
// sub-block is coded with outputSize = its own size
static PstreamJob ps_job(BlockJob& J, int q)
{
    sub_scratch(J, q);
    return PstreamJob{J.views[q].first_seen, J.views[q].nsym, J.size[q], J.ps_of(q), (size_t)(J.poff[q + 1] - J.poff[q]), J.scratch[q].get(), J.size[q]};
}
// ... and what its coder returned: a sub-block that did not compress would be stored raw, which needs the run arrays — the block is redone
static void ps_record(BlockJob& J, int q, int r)
{
    if (r < 0) J.redo.store(true, std::memory_order_relaxed);
    J.sub_res[q] = r < 0 ? J.size[q] : r;
}

// BSCGPU_OPT_DEVICE_RC: the sub-block streams of a device-model block through the device's range coder (rangecoder.hip), one launch on
// the context's stream straight from the device's p stream; only the coded bytes come down, into the sub-blocks' scratch buffers, and
// host_finalize frames them as ever.  Every sub-block is coded with outputSize = its own size (coder.cpp:159-240), as host_encode_sub
// does; one that ends LIBBSC_NOT_COMPRESSIBLE sets redo in the same way.  The output regions lie in the sorter's first key buffer, which
// nothing reads once the p stream exists (8 max_n bytes; the regions take n + 8 * 128 at most).
static int device_rc_block(BlockJob& J, int psbuf)
{
    bscgpu_ctx* c = J.c;
    const int nb = J.nblocks;
    std::vector<uint32_t> prefix;
    bscgpu_rc_stream S[8];
    int res[8];
    uint32_t off = 0;
    for (int b = 0; b < nb; ++b) {
        uint8_t fs[256]; int nsym = 0;
        qlfc_front_first_seen(J.first_run + 256 * (size_t)b, fs, &nsym);
        const size_t at = prefix.size();
        prefix.resize(at + BSCGPU_RC_PREFIX_MAX);
        const int np = bscgpu_rc_prefix(fs, nsym, J.size[b], J.coder, prefix.data() + at, BSCGPU_RC_PREFIX_MAX);
        if (np < 0) return np;
        prefix.resize(at + (size_t)np);
        S[b].body = J.ps_packed ? (int64_t)J.pbase[b] : (int64_t)J.poff[b];
        S[b].count = J.poff[b + 1] - J.poff[b];
        S[b].prefix = (uint32_t)at; S[b].nprefix = (uint32_t)np;
        S[b].out_off = off; S[b].out_size = J.size[b];
        off += ((uint32_t)J.size[b] + 64u + 63u) & ~63u;
    }
    if ((size_t)off > (size_t)8 * (size_t)c->max_n) return LIBBSC_NOT_SUPPORTED;
    uint8_t* dOut = reinterpret_cast<uint8_t*>(c->kA);
    // (one stream per wavefront: with a block's 2 .. 8 streams the wave-uniform chain is the fastest shape measured)
    int rc = rc_encode_device(c, ps_form(J), devcoder_pstream_ptr(c, psbuf), prefix.data(), (int)prefix.size(), S, nb, dOut, res, 1);
    if (rc < 0) return rc;
    for (int b = 0; b < nb; ++b) {
        sub_scratch(J, b);
        ps_record(J, b, res[b]);
        if (res[b] < 0) continue;
        if (hipMemcpyAsync(J.scratch[b].get(), dOut + S[b].out_off, (size_t)res[b], hipMemcpyDeviceToHost, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
    }
    if (ctx_sync(c) != hipSuccess) return LIBBSC_GPU_ERROR;
    return LIBBSC_NO_ERROR;
}

// ---- the stream of a device-model block on its way to the host ---------------------------------------------------------------------
// Where sub-block b's piece lies is DcBlockSchedule's (dc_block_plan.h), for a block in segments and for one modelled in one go alike:
// the job's poff / pbase are the schedule's -> the entries the landing zone must hold
static size_t ps_layout(BlockJob& J, const DcBlockSchedule& plan)
{
    for (int b = 0; b <= J.nblocks; ++b) { J.poff[b] = (u32)plan.poff_of(b); J.pbase[b] = (u32)plan.pbase_of(b); }
    return ((size_t)plan.zone_bytes() + 1u) / 2u + 64;
}

// The one sender of pieces from a device stream buffer (ps[pb], synchronised behind the last kernel that wrote it) to the slot's landing
// zone, which exists (ctx_ensure_pstream_slot).  A piece is NOT waited for here: the next segment's kernels and the next block's sort
// overlap it, the coder task of sub-blocks b.. waits for ITS pieces (J.ps_landed; 366 MB take 7-14 ms over PCIe).
// Which engine moves them is decided once per block: hipMemcpyAsync is a DMA-engine copy on the system's HIP runtime but a 256-workgroup
// copy KERNEL on the runtime a torch process carries (dma_copy.h), so the pieces go to the HSA runtime's DMA copy directly and complete
// HSA signals; hipMemcpyAsync on the copy stream + an event per piece remain where that is not possible (or BSC_D2H_DMA=0).  Either way
// the buffer's guard (c->ps_guard_sig / c->ps_guard: the next model run into it waits) is what its pieces complete: their signals, or
// the event of the last piece issued from it.  finish() records the slot's copy_ev directly behind that event with nothing between
// them, so for the block's last buffer a wait on either is the same wait.
// The engine refusing a piece (its queue is full): that piece alone goes through HIP behind everything queued so far, is waited for and
// counts as landed by the host (ps_sig 0), for a whole block as for a segment.  (Until this sender a whole block sent its whole stream
// again through HIP instead: other copies, the same bytes.  No test reaches this exit without exhausting the engine's queue on purpose.)
struct PsSender {
    BlockJob& J; bscgpu_ctx* c; bool dma; int issued = 0;             // issued: sub-blocks whose piece is in flight or has landed
    PsSender(BlockJob& job, bscgpu_ctx* ctx) : J(job), c(ctx), dma(dma_available() && job.slot->hps_dev != nullptr)
    {
        for (int b = 0; b < 8 && dma; ++b) dma = J.slot->part_sig[b] != 0;
        J.ps_dma = dma; J.ps_ready = nullptr;
    }
    // buffer pb is about to send: its guards are the pieces issued from here on
    void begin(int pb) { c->ps_guard[pb] = nullptr; for (int b = 0; b < 8; ++b) c->ps_guard_sig[pb][b] = 0; }
    // sub-block s's piece: len bytes at src (device, in ps[pb]) to byte dst of the zone; len 0: nothing to copy (the host put it there)
    int piece(int s, int pb, const uint8_t* src, size_t dst, size_t len)
    {
        uint8_t* const zone = reinterpret_cast<uint8_t*>(J.slot->hps);
        issued = s + 1;
        if (dma) {
            J.ps_sig[s] = 0;
            if (len == 0) return LIBBSC_NO_ERROR;
            if (dma_d2h((uint8_t*)J.slot->hps_dev + dst, src, len, J.slot->part_sig[s]) == 0) { J.ps_sig[s] = c->ps_guard_sig[pb][s] = J.slot->part_sig[s]; return LIBBSC_NO_ERROR; }
            return settle() && hipMemcpyAsync(zone + dst, src, len, hipMemcpyDeviceToHost, c->stream) == hipSuccess && ctx_sync(c) == hipSuccess ? LIBBSC_NO_ERROR : LIBBSC_GPU_ERROR;
        }
        if ((len > 0 && hipMemcpyAsync(zone + dst, src, len, hipMemcpyDeviceToHost, c->copy_stream) != hipSuccess) ||
            hipEventRecord(J.slot->part_ev[s], c->copy_stream) != hipSuccess) return LIBBSC_GPU_ERROR;
        J.ps_part[s] = c->ps_guard[pb] = J.slot->part_ev[s];
        return LIBBSC_NO_ERROR;
    }
    // every piece of segment g, which lies in ps[pb]; host_put: the host has packed the segment into the zone itself
    int segment(const DcBlockSeg& g, int pb, bool host_put = false)
    {
        const uint8_t* dps = reinterpret_cast<const uint8_t*>(devcoder_pstream_ptr(c, pb));
        int rc = LIBBSC_NO_ERROR;
        begin(pb);
        for (int s = g.s0, k = 0; s < g.s1 && rc >= 0; ++s, ++k) rc = piece(s, pb, dps + g.src[k], (size_t)g.dst[k], host_put ? 0 : (size_t)g.len[k]);
        return rc;
    }
    // everything issued so far has landed (before the host writes a piece itself, and before the block is given up)
    bool settle()
    {
        bool ok = dma || hipStreamSynchronize(c->copy_stream) == hipSuccess;
        for (int b = 0; dma && b < issued; ++b) ok = (J.ps_sig[b] == 0 || dma_wait(J.ps_sig[b]) == 0) && ok;
        return ok;
    }
    // the block's last piece has been issued
    int finish()
    {
        if (!dma && hipEventRecord(J.slot->copy_ev, c->copy_stream) != hipSuccess) return LIBBSC_GPU_ERROR;
        if (!dma) J.ps_ready = J.slot->copy_ev;
        return LIBBSC_NO_ERROR;
    }
};

// The device model of a block on a context whose arena is divided (BSCGPU_OPT_DC_ARENA_DIV > 1; DESIGN §3.6, "A block in sub-block
// segments"): facts, plan, then the segments in order, segment i into the device stream buffer ps_toggle names behind that buffer's
// guard, its pieces through the sender to the block's one landing zone while the next segment's kernels run.  Returns what
// devcoder_pstream returns; J.poff / J.pbase / J.ps_packed / *ndec are the block's.  *sent = false: the plan is one segment, which lies
// in ps[ps_toggle] as devcoder_pstream leaves a block (a void packed form: 16-bit entries), and the caller goes on as ever.  *sent =
// true: several segments, all pieces issued.  A segment that declines declines the block (what is in flight lands first); one whose
// packed form is void comes down as 16-bit entries and is packed into place by the host (dc_pack13_host): the block stays in one form.
static int devcoder_block_in_segments(BlockJob& J, u32 m, const int* maxr, u32* ndec, bool* sent)
{
    bscgpu_ctx* c = J.c;
    DcBlock B;
    const FrontBufs fb = front_bufs(c);
    int rc = devcoder_block_begin(c, fb.sym, fb.rank, fb.start, m, (u32)J.n, J.nblocks, J.start, J.size,
                                  J.run_first, maxr, J.coder, true, &B);
    if (rc < 0) return rc;
    const DcBlockSchedule& plan = B.plan;
    *ndec = (u32)plan.decisions();
    const size_t zone_entries = ps_layout(J, plan);
    if (plan.segments() == 1) {
        bool host_packed = false;
        rc = devcoder_block_segment(c, &B, plan.segment(0), c->ps_toggle, &host_packed);
        J.ps_packed = B.packed && !host_packed;
        return rc;
    }
    J.ps_packed = B.packed;
    if (ctx_ensure_pstream_slot(c, *J.slot, zone_entries) != LIBBSC_NO_ERROR) return LIBBSC_NOT_SUPPORTED;    // (as an arena that does not fit)
    PsSender send(J, c);
    std::vector<uint16_t> void_entries;
    for (int i = 0; i < plan.segments(); ++i) {
        const int pb = c->ps_toggle;
        const DcBlockSeg g = plan.segment(i);
        bool host_packed = false;
        rc = devcoder_block_segment(c, &B, g, pb, &host_packed);
        if (rc < 0) { (void)send.settle(); return rc; }
        if (host_packed) {
            void_entries.resize((size_t)g.expect);
            if (hipMemcpyAsync(void_entries.data(), devcoder_pstream_ptr(c, pb), (size_t)g.expect * 2, hipMemcpyDeviceToHost, c->stream) != hipSuccess || ctx_sync(c) != hipSuccess ||
                !send.settle() || !plan.pack_void(g, void_entries.data(), reinterpret_cast<uint8_t*>(J.slot->hps))) return LIBBSC_GPU_ERROR;
        }
        rc = send.segment(g, pb, host_packed);
        if (rc < 0) return rc;
        c->ps_toggle = pb ^ 1;
    }
    *sent = true;
    return send.finish();
}

// ---- the GPU stage of one block: its steps (the decisions among them: dc_block_plan.h) ---------------------------------------------
// sort: the BWT with its secondary indexes, or a sort transform, into c->dL
static int stage_sort(BlockJob& J, int blockSorter)
{
    bscgpu_ctx* c = J.c;
    const int n = J.n;
    J.num_indexes = 0;
    if (blockSorter == LIBBSC_BLOCKSORTER_BWT) {
        const int r = aux_rate(n);
        uint32_t I[256];
        int64_t primary = 0;
        const int rc = bwt_device(c, (const u8*)J.dInput, c->dL, n, r, I, &primary);
        if (rc < 0) return rc;
        J.index = (int)primary;
        J.num_indexes = (n - 1) / r;
        for (int t = 0; t < J.num_indexes; ++t) J.indexes[t] = (int)I[t + 1] - 1;
    } else {
        const int rc = st_device(c, (const u8*)J.dInput, c->dL, n, blockSorter, &J.index);
        if (rc < 0) return rc;
    }
    if (J.n_orig < 64 * 1024) J.num_indexes = 0;              // libbsc.cpp:290 (the original size decides)
    return LIBBSC_NO_ERROR;
}

// model, decide: static coder on a block with several sub-blocks: the adaptive model runs on the GPU too (devcoder.hip) and only the
// probability stream crosses PCIe; anything that path declines falls back to the run arrays + host model
// (an LZP-preprocessed block — the reference CLI's default, bsc.cpp:73-75 — is just another byte block to the sorter and the model;
// its LZP output stays alive until the block is done, because a redo on the host model uploads it again)
// (the fast coder, -e0, runs on the same device machinery: its one counter per decision is the static coder's char family with
// other update maps — devcoder.hip: dc_fast_run; BSC_DEVICE_CODER_FAST=0 keeps it on the host)
static bool model_tries(const BlockJob& J, bool allow_devcoder)
{
    static const bool dc_fast = [] { const char* e = getenv("BSC_DEVICE_CODER_FAST"); return e ? atoi(e) != 0 : true; }();
    return dc_block_tries_model(allow_devcoder, devcoder_enabled(), J.coder == LIBBSC_CODER_QLFC_STATIC, J.coder == LIBBSC_CODER_QLFC_FAST && dc_fast,
                                J.nblocks, J.n, devcoder_min_n());
}
// model, run and land -> < 0, or *took: the block is the device model's (else its run arrays are still to go down)
static int stage_model(BlockJob& J, u32 m, bool* took)
{
    bscgpu_ctx* c = J.c;
    *took = false;
    if (dc_block_runs_too_dense(m, J.n)) return LIBBSC_NO_ERROR;
    // run: whole into ps[pb], or in segments (sent: its pieces are on their way already)
    int maxr[8], packed = 0;
    dc_max_rank_table(J.first_run, J.nblocks, maxr);
    u32 ndec = 0;
    const int pb = c->ps_toggle;
    bool sent = false;
    const FrontBufs fb = front_bufs(c);
    const int mrc = c->dc_arena_div > 1 ? devcoder_block_in_segments(J, m, maxr, &ndec, &sent)
                  : devcoder_pstream(c, fb.sym, fb.rank, fb.start, m, (u32)J.n, J.nblocks,
                                     J.run_first, maxr, &ndec, J.poff, nullptr, pb, J.coder, &packed);
    if (c->dc_arena_div == 1) J.ps_packed = packed != 0;
    // the whole stream lies in ps[pb]: its layout there = in the landing zone
    const bool whole = mrc == LIBBSC_NO_ERROR && !sent;
    const DcBlockSchedule lay = whole ? DcBlockSchedule::whole(J.poff, J.nblocks, J.ps_packed) : DcBlockSchedule();
    const size_t zone_entries = whole ? ps_layout(J, lay) : 0;
    // (a pinned landing zone that cannot be had is a reason to take the host model, like an arena that does not fit)
    const bool zone = whole && !c->device_rc && ctx_ensure_pstream_slot(c, *J.slot, zone_entries) == LIBBSC_NO_ERROR;
    int rc = LIBBSC_NO_ERROR;
    switch (dc_block_verdict(mrc, sent, c->device_rc != 0, zone)) {
    case DC_BLOCK_HOST_MODEL: return LIBBSC_NO_ERROR;
    case DC_BLOCK_ERROR: return mrc;
    case DC_BLOCK_SENT: break;
    case DC_BLOCK_DEVICE_RC:
        // the range coder runs here as well: the stream stays in HBM (its buffer is free again when this returns: no guard, no toggle)
        rc = device_rc_block(J, pb);
        if (rc < 0) return rc;
        J.rc_done = true; ++c->cnt_device_rc;
        break;
    case DC_BLOCK_LANDED: {
        // one segment through the sender: one copy per sub-block, none waited for
        PsSender send(J, c);
        rc = send.segment(lay.segment(0), pb);
        if (rc >= 0) rc = send.finish();
        if (rc < 0) return rc;
        c->ps_toggle = pb ^ 1;
        break; }
    }
    // the block is the device model's: the host codes from the landing zone, or has nothing left to code
    *took = J.use_ps = true; J.ps = J.rc_done ? nullptr : J.slot->hps; J.ndec = ndec;
    g_count_devmodel.fetch_add(1, std::memory_order_relaxed);
    if (J.lz || (J.dev_lzp && block_mode_has_lzp(J.mode))) g_count_devmodel_lzp.fetch_add(1, std::memory_order_relaxed);
    return LIBBSC_NO_ERROR;
}

// small block stored | adler | sort | front (split and runs) | model | the run arrays down if the model did not take the block
static int gpu_stage(BlockJob& J, int blockSorter, bool allow_devcoder = true)
{
    CtxTimer tm_stage("gpu_stage of one block");
    J.sorter = blockSorter; J.use_ps = false; J.ps_packed = false; J.rc_done = false; J.redo.store(false, std::memory_order_relaxed);
    bscgpu_ctx* c = J.c;
    const int n = J.n;
    if (hipSetDevice(c->device) != hipSuccess) return LIBBSC_GPU_ERROR;
    if (n <= LIBBSC_HEADER_SIZE) {
        unsigned char tmp[LIBBSC_HEADER_SIZE + 1];
        if (n > 0 && hipMemcpy(tmp, J.dInput, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return LIBBSC_GPU_ERROR;
        J.result = bsc_store(tmp, J.output, n, J.features);
        J.stored_small = true;
        return LIBBSC_NO_ERROR;
    }
    auto t0 = clk::now();
    int rc = J.have_adler ? LIBBSC_NO_ERROR : adler32_device(c, (const u8*)J.dInput, n, &J.adler_data);
    if (rc < 0) return rc;
    c->stage_ms[0] = ms_since(t0);

    t0 = clk::now();
    rc = stage_sort(J, blockSorter);
    if (rc < 0) return rc;
    c->stage_ms[1] = ms_since(t0);

    // QLFC front half on the GPU (sub-block split, runs, ranks); only the run arrays (+ L for the rare raw sub-block) cross PCIe, into
    // this job's pinned slot: at once where the block does not try the device model, after it where the model did not take the block
    t0 = clk::now();
    J.nblocks = coder_num_blocks(n);
    rc = qlfc_front_split(c, c->dL, (u32)n, J.nblocks, J.start, J.size);
    if (rc < 0) return rc;
    u32 m = 0;
    const bool try_dc = model_tries(J, allow_devcoder);
    bool took = false;
    rc = qlfc_front_runs(c, c->dL, (u32)n, J.nblocks, J.start, &m, J.run_first, J.first_run, *J.slot, !try_dc);
    if (rc >= 0 && try_dc) rc = stage_model(J, m, &took);
    if (rc >= 0 && try_dc && !took) rc = qlfc_front_copy_runs(c, m, *J.slot);
    if (rc < 0) return rc;
    c->stage_ms[2] = ms_since(t0);
    return LIBBSC_NO_ERROR;
}

static void host_prepare(BlockJob& J)
{
    for (int b = 0; b < J.nblocks; ++b) {
        RunView& V = J.views[b];
        V = RunView();
        V.sym = J.slot->hsym + J.run_first[b]; V.rank = J.slot->hrank + J.run_first[b]; V.start = J.slot->hstart + J.run_first[b];
        V.count = J.run_first[b + 1] - J.run_first[b];
        V.end = (u32)(J.start[b] + J.size[b]);
        // alphabet in order of first appearance = symbols sorted by the index of their first run
        std::pair<u32, int> order[256]; int k = 0;
        for (int s = 0; s < 256; ++s) if (J.first_run[b * 256 + s] != 0xffffffffu) order[k++] = {J.first_run[b * 256 + s], s};
        std::sort(order, order + k);
        V.nsym = k;
        for (int i = 0; i < k; ++i) V.first_seen[i] = (uint8_t)order[i].second;
    }
}

// The sorted bytes of a sub-block, rebuilt from its run arrays (needed only when a sub-block has to be stored raw; this is
// why the sorted block itself never crosses PCIe).
static void expand_runs(const RunView& V, int sub_start, uint8_t* dst)
{
    for (uint32_t j = 0; j < V.count; ++j) memset(dst + (V.start[j] - (uint32_t)sub_start), V.sym[j], V.len(j));
}

// One sub-block, from its run arrays or — a device-model block — from its probability stream.  A stream coder's task waits for the
// arrival of its last sub-block's piece of the stream; if that did not land the block is redone on the host model.
static void host_encode_sub(BlockJob& J, int b)
{
    if (!J.use_ps) {
        sub_scratch(J, b);
        const int r = qlfc_encode_runs(J.views[b], J.size[b], J.scratch[b].get(), J.size[b], J.coder);      // outputSize = its own size, as in ps_job
        J.sub_res[b] = (r < 0) ? J.size[b] : r;
        return;
    }
    const PstreamJob P = ps_job(J, b);
    if (J.rc_done) return;
    ps_record(J, b, J.ps_landed(b) ? qlfc_encode_pstream(ps_form(J), P) : LIBBSC_NOT_COMPRESSIBLE);
}

// two sub-blocks of a device-model block in one interleaved range-coder loop (b even)
static void host_encode_pair(BlockJob& J, int b)
{
    if (!J.use_ps || b + 1 >= J.nblocks) { host_encode_sub(J, b); if (b + 1 < J.nblocks) host_encode_sub(J, b + 1); return; }
    if (J.rc_done) return;
    const PstreamJob P[2] = {ps_job(J, b), ps_job(J, b + 1)};
    int r[2] = {LIBBSC_NOT_COMPRESSIBLE, LIBBSC_NOT_COMPRESSIBLE};
    if (J.ps_landed(b + 1)) qlfc_encode_pstream_pair(ps_form(J), P[0], P[1], &r[0], &r[1]);
    ps_record(J, b, r[0]); ps_record(J, b + 1, r[1]);
}

// How the eight sub-blocks of a device-model block are coded on the host (EPYC 9575F, the coding loops alone on one quiet thread, per 64 MiB
// bench block: tools/rc_host_bench.cpp, profiles/r05/host_coder_on_box_cpu.txt; round 4's figures in brackets):
//   8  all eight in the lanes of one SIMD range-coder loop (qlfc_encode_pstream_x8): one task of 96 ms [104] with AVX-512VL (126 with AVX2)
//   2  four tasks of two interleaved scalar coders: 48 ms each [54], 0.19 CPU-s
//   1  eight tasks of one scalar coder: 35 ms each [46], 0.28 CPU-s [0.37]
// bscgpu_coder_task_shape is the rule (a pure function, unit-tested on CPU); ps_group feeds it.  BSC_RC_SIMD=8 / 0 forces eight lanes /
// pairs everywhere, BSC_RC_ADAPTIVE=1 turns the idle test on (round 3-4's default: pairs for a block that finds >= 4 CPUs idle; off,
// every block that is not marked low-latency is one eight-lane task).
static int ps_simd_env()
{
    static const int mode = [] {
        if (const char* e = getenv("BSC_RC_SIMD")) return atoi(e) == 8 ? 8 : 0;
        if (const char* e = getenv("BSC_RC_X8")) return atoi(e) != 0 ? 8 : 0;
        return -1;
    }();
    return mode;
}
static int default_coder_threads();
static std::atomic<int> g_sync_callers{0};            // synchronous host stages running right now (bsc_compress / bscgpu_compress_device callers)
static bool cpu_has_avx512vl() { static const bool has = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512vl"); return has; }
// forced: -1 none, 8 / 0 (BSC_RC_SIMD); low_latency: a synchronous call, or the caller marked the block (BSCGPU_FEATURE_LOW_LATENCY);
// pool_free: CPUs of the coder pool's budget with nothing to do when the block is queued, -1 for a synchronous call (which starts
// its own threads: sync_cpus = CPUs / synchronous callers running); wide_simd: AVX-512VL; adaptive: BSC_RC_ADAPTIVE.
extern "C" BSCGPU_API int bscgpu_coder_task_shape(int forced, int low_latency, int pool_free, int sync_cpus, int wide_simd, int adaptive)
{
    if (forced >= 0) return forced == 8 ? 8 : 2;
    if (low_latency) {
        // a pipe's block marked low-latency: pairs — the blocks around it are still being coded, eight more tasks would queue behind
        // them — unless eight CPUs of the pool have nothing to do: then eight single-stream tasks all start at once and the block is out
        // after 35 instead of 48 ms (round 5: the single-stream loop lost its mispredicted branch and two cycles of its chain; before that
        // its tasks took as long as the pairs' and the threshold was 12)
        if (pool_free >= 0) return pool_free >= 8 ? 1 : 2;
        // a synchronous call: eight threads only if its share of the CPUs has room for them (the reference CLI calls bsc_compress from
        // an OpenMP team: four callers x eight threads on 16 CPUs took 1.29 s for 8 x 64 MiB, sized by share 1.15 s)
        return sync_cpus >= 8 ? 1 : 2;
    }
    if (!wide_simd) return 2;
    // A pipe's block: the eight-lane task costs half the CPU time of four pair tasks but takes 96 instead of 48 ms.  While the pool has
    // four CPUs with nothing to do the pairs cost nothing and the block is out 40 ms earlier (a short job is mostly pipeline fill and
    // drain); when the coder threads are busy — many GPUs per host, a small quota — every block is one eight-lane task and the pool's
    // throughput is what counts.
    return (adaptive && pool_free >= 4) ? 2 : 8;
}
static int ps_group(const BlockJob& J)
{
    if (!J.use_ps || J.nblocks != 8) return 2;
    // Round 5: off by default.  Pairs for blocks that find idle CPUs double the CPU time of exactly the blocks at the HEAD of a job, and
    // that work is still queued when the tail arrives: at the driver's 20 steps, one box, three alternating runs each — 3396 / 3572 / 3971
    // MB/s with the idle test, 3841 / 3862 / 4018 without; 160 steps the same (5257 / 5205) at 0.127 instead of 0.164 CPU-s per block.
    // The job's tail is still coded as short tasks: its blocks are marked low-latency by whoever knows where the job ends.
    static const int adaptive = [] { const char* e = getenv("BSC_RC_ADAPTIVE"); return e ? atoi(e) : 0; }();
    static const int cpus = default_coder_threads();
    const int callers = g_sync_callers.load(std::memory_order_relaxed);
    if ((J.features & BSCGPU_FEATURE_URGENT) && ps_simd_env() < 0) return 1;       // the caller's word: eight single-stream tasks
    // An announced job (bscgpu_coder_pool_expect): the shape follows the order in which GPU stages END, which is what decides when a
    // block's coding can start — not the order in which the caller submitted them (with several contexts interleaving on the GPU the
    // two differ by 100 ms: round 6's task timeline had blocks submitted 8th..10th from last end their GPU stage 60 ms before the
    // job's last one, take an eight-lane task of 110-120 ms each, and finish the job).  The last block: eight single-stream tasks
    // (35 ms); the few before it: pairs (50 ms); everything earlier ends in time as one eight-lane task (half the CPU time).
    if (J.tail_r >= 0 && ps_simd_env() < 0 && cpu_has_avx512vl()) {
        static const int tail_singles = [] { const char* e = getenv("BSC_TAIL_SINGLES"); return e ? atoi(e) : 1; }();
        // how many blocks before the last as pairs: two fewer than the contexts that interleave on a GPU (measured: 5 contexts: 3 > 4 > 5 pair-blocks;
        // 6 contexts: 4 = 5 > 3 — profiles/r06/pool_affinity.txt, short_job_tail.txt); BSC_TAIL_PAIRS sets it by hand
        static const int tail_pairs_env = [] { const char* e = getenv("BSC_TAIL_PAIRS"); return e ? atoi(e) : -1; }();
        const int tail_pairs = tail_pairs_env >= 0 ? tail_pairs_env : (J.tail_pipes - 2 < 2 ? 2 : J.tail_pipes - 2 > 6 ? 6 : J.tail_pipes - 2);
        const int gp = J.tail_gpus > 0 ? J.tail_gpus : 1;               // GPUs feeding the pool: that many GPU stages end per block time
        if (J.tail_r < tail_singles * gp) return 1;
        if (J.tail_r < (tail_singles + tail_pairs) * gp) return 2;
        if (!(J.features & BSCGPU_FEATURE_LOW_LATENCY)) return 8;
    }
    return bscgpu_coder_task_shape(ps_simd_env(), ((J.features & BSCGPU_FEATURE_LOW_LATENCY) || !J.pipelined) ? 1 : 0, J.pool_free,
                                   cpus / (callers > 1 ? callers : 1), cpu_has_avx512vl() ? 1 : 0, adaptive);
}
// sub-blocks b .. b + g - 1 of a device-model block, g = ps_group(J)
static void host_encode_group(BlockJob& J, int b)
{
    const int g = J.ps_g;
    if (J.rc_done) return;                          // coded in the GPU stage (device_rc_block)
    if (g == 2) { host_encode_pair(J, b); return; }
    if (g == 1) { host_encode_sub(J, b); return; }
    PstreamJob P[8];
    for (int k = 0; k < g; ++k) P[k] = ps_job(J, b + k);
    int r[8];
    if (!J.ps_landed(b + g - 1)) std::fill(r, r + g, (int)LIBBSC_NOT_COMPRESSIBLE);
    else if (!qlfc_encode_pstream_x8(ps_form(J), P, r)) {
        for (int k = 0; k < g; k += 2) host_encode_pair(J, b + k);      // a stream near its budget: the exact scalar coders
        return;
    }
    for (int k = 0; k < g; ++k) ps_record(J, b + k, r[k]);
}

static void write_stored(BlockJob& J)
{
    if (J.hInput) { J.result = J.inplace ? LIBBSC_NOT_COMPRESSIBLE : bsc_store(J.hInput, J.output, J.n_orig, J.features); return; }   // libbsc.cpp:188, :315
    J.result = store_from_device(J.c, J.dRaw ? J.dRaw : J.dInput, J.output, J.n_orig, J.adler_data);
}

// result: the payload's bytes at block_body(J.output), or the coder's negative code
static void write_header_and_trailer(BlockJob& J, int result)
{
    J.result = block_finish_coded(J.output, J.n_orig, result, J.mode, J.index, J.indexes, J.num_indexes, J.adler_data);
    if (J.result == LIBBSC_NOT_COMPRESSIBLE) write_stored(J);
}

namespace {
struct RunsFetch : RawFetch {                                       // a sub-block stored raw is rebuilt from its runs
    const RunView* views; const int* st; const int* sz; int nb;
    RunsFetch(const RunView* views_, const int* st_, const int* sz_, int nb_) : views(views_), st(st_), sz(sz_), nb(nb_) {}
    int operator()(int start, int size, uint8_t* dst) override
    {
        for (int q = 0; q < nb; ++q) if (st[q] == start && sz[q] == size) { expand_runs(views[q], start, dst); return 0; }
        return LIBBSC_BAD_PARAMETER;
    }
};
}

// sub-block b of a block whose sub-blocks were coded on their own: once from its scratch buffer, or, kept raw, expanded from its runs
static int put_coded_sub(const BlockJob& J, int b, uint8_t* dst)
{
    if (J.sub_res[b] != J.size[b]) memcpy(dst, J.scratch[b].get(), (size_t)J.sub_res[b]);
    else expand_runs(J.views[b], J.start[b], dst);
    return 0;
}

// frame the independently coded sub-blocks (nblocks > 1, MULTITHREADING semantics)
static void host_finalize_parallel(BlockJob& J)
{
    write_header_and_trailer(J, frame_parallel(block_body(J.output), J.n, J.nblocks, J.size, J.sub_res, [&J](int b, uint8_t* dst) { return put_coded_sub(J, b, dst); }));
}

// every block with more than one sub-block is coded as independent per-sub-block tasks, whatever the caller's
// MULTITHREADING flag says: the flag selects the reference's *framing rules* (coder.cpp:111 serial / :159 parallel), which
// differ only in corner cases, not whether this library may use its coder threads.
static bool job_uses_tasks(const BlockJob& J) { return !J.stored_small && J.nblocks > 1; }

// the block's sub-blocks through the strictly serial coder (coder.cpp:111-155) on this thread
static void host_code_serially(BlockJob& J)
{
    RunsFetch fetch(J.views, J.start, J.size, J.nblocks);
    unsigned char* buffer = (unsigned char*)bsc_malloc((size_t)J.n + 4096);
    if (!buffer) { J.result = LIBBSC_NOT_ENOUGH_MEMORY; return; }
    const int result = coder_compress_views(J.views, J.nblocks, J.start, J.size, J.n, buffer, J.coder, J.features & ~LIBBSC_FEATURE_MULTITHREADING, fetch);
    if (result >= 0) memcpy(block_body(J.output), buffer, (size_t)result);
    bsc_free(buffer);
    write_header_and_trailer(J, result);
}

// Serial framing rules (coder.cpp:111-155) applied to sub-blocks that were coded independently, each with an output
// budget of its own size: where serial_verdict (container.h) says that this is what the serial coder would have produced —
// always, unless the block is close to incompressible — they are framed as they are.  Otherwise the block is simply coded
// again serially.
static void host_finalize_serial(BlockJob& J)
{
    switch (serial_verdict(J.n, J.nblocks, J.size, J.sub_res)) {
    case SERIAL_NOT_EXACT:
        if (J.use_ps) J.redo.store(true, std::memory_order_relaxed); else host_code_serially(J);
        return;
    case SERIAL_INCOMPRESSIBLE:
        write_header_and_trailer(J, LIBBSC_NOT_COMPRESSIBLE);
        return;
    case SERIAL_EXACT:
        write_header_and_trailer(J, subtable_write(block_body(J.output), J.nblocks, J.size, J.sub_res, [&J](int b, uint8_t* dst) { return put_coded_sub(J, b, dst); }));
    }
}

static void host_finalize(BlockJob& J)
{
    if (J.use_ps && J.redo.load(std::memory_order_relaxed)) { J.result = LIBBSC_GPU_ERROR; return; }   // finished later by redo_on_host_model(), which sets the result; an error until then
    if (J.features & LIBBSC_FEATURE_MULTITHREADING) host_finalize_parallel(J); else host_finalize_serial(J);
}

// whole host stage on the calling thread (+ its own sub-block threads): the synchronous entry points
static void host_stage(BlockJob& J)
{
    if (J.stored_small) return;
    host_prepare(J);
    if (job_uses_tasks(J)) {
        struct Caller { Caller() { g_sync_callers.fetch_add(1, std::memory_order_relaxed); } ~Caller() { g_sync_callers.fetch_sub(1, std::memory_order_relaxed); } } caller;
        if (J.use_ps) { const int g = J.ps_g = ps_group(J); run_tasks(J.nblocks / g, [&J, g](int t) { host_encode_group(J, g * t); }); }
        else run_tasks(J.nblocks, [&J](int b) { host_encode_sub(J, b); });
        host_finalize(J);
        return;
    }
    host_code_serially(J);
}

// Host-resident block -> job, part 1 (no GPU involved): optional LZP on the host (lzp.cpp:798 semantics).  `sorter` may be
// changed (a tiny LZP output is always BWT-sorted, libbsc.cpp:277-281).
// device_lzp (BSCGPU_OPT_DEVICE_LZP): a block with LZP whose parameters the device stage takes is left raw here — stage_host_h2d
// uploads it and runs the stage (stage_device_lzp); *declined says that the block has LZP and the stage does not take it.
static bool device_lzp_takes(int lzpHashSize) { return lzpHashSize >= 10 && lzpHashSize <= lzp::STAGED_MAX_HASH; }
static int stage_host_lzp(BlockJob& J, const unsigned char* input, unsigned char* output, int n,
                          int lzpHashSize, int lzpMinLen, int* sorter, int coder, int features, int mode,
                          bool device_lzp = false, bool* declined = nullptr)
{
    int lzSize = n;
    J.lz.reset();
    J.dev_lzp = false; J.dRaw = nullptr;
    if (declined) *declined = device_lzp && block_mode_has_lzp(mode) && !device_lzp_takes(lzpHashSize);
    if (device_lzp && block_mode_has_lzp(mode) && device_lzp_takes(lzpHashSize)) {
        J.dev_lzp = true; J.lzp_hash = lzpHashSize; J.lzp_min = lzpMinLen; J.mode_with_lzp = mode;
    } else if (block_mode_has_lzp(mode)) {
        J.lz = std::unique_ptr<unsigned char, void (*)(void*)>((unsigned char*)bigbuf_get((size_t)n), bigbuf_put);   // (par.h: a few block-sized buffers are kept)
        if (!J.lz) return LIBBSC_NOT_ENOUGH_MEMORY;
        const int r = lzp_compress(input, J.lz.get(), n, lzpHashSize, lzpMinLen, features);
        if (r < LIBBSC_NO_ERROR) { mode = block_mode_without_lzp(mode); J.lz.reset(); }            // libbsc.cpp:266-269: the block goes on without LZP
        else lzSize = r;
    }
    if (lzSize <= LIBBSC_HEADER_SIZE) { *sorter = LIBBSC_BLOCKSORTER_BWT; mode = block_mode_with_sorter(mode, LIBBSC_BLOCKSORTER_BWT); }
    J.hInput = input; J.output = output; J.n = lzSize; J.n_orig = n; J.inplace = (input == output);
    J.coder = coder; J.features = features; J.mode = mode; J.stored_small = false; J.result = 0; J.have_adler = false;
    if (J.lz) { J.adler_data = adler32(input, (size_t)n); J.have_adler = true; }
    return LIBBSC_NO_ERROR;
}
// The LZP stage of a raw block in HBM (c->dT after an upload, or J.dRaw): Adler-32 of the original, then the sorter's input into c->dL.
// A block the stage finds not compressible goes on without LZP (libbsc.cpp:266-269).  Repeatable: a redo runs it again.
static int stage_device_lzp(BlockJob& J, bscgpu_ctx* c)
{
    const u8* raw = J.dRaw ? (const u8*)J.dRaw : c->dT;
    int rc = adler32_device(c, raw, J.n_orig, &J.adler_data);
    if (rc < 0) return rc;
    J.have_adler = true;
    const int r = lzp_device(c, raw, c->dL, J.n_orig, J.lzp_hash, J.lzp_min, J.features, false);
    ++c->cnt_lzp_blocks;
    g_count_device_lzp.fetch_add(1, std::memory_order_relaxed);
    if (r < 0 && r != LIBBSC_NOT_COMPRESSIBLE) return r;
    // (a coded block is 1 + 4 + the tail behind `limit`, 36 bytes and more: never as small as a header, so the sorter stays the caller's)
    if (r >= 0 && r <= LIBBSC_HEADER_SIZE) return LIBBSC_GPU_ERROR;
    if (r < 0 && hipMemcpyAsync(c->dL, raw, (size_t)J.n_orig, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
    J.n = r < 0 ? J.n_orig : r;
    J.mode = r < 0 ? block_mode_without_lzp(J.mode_with_lzp) : J.mode_with_lzp;
    J.dInput = c->dL;
    return LIBBSC_NO_ERROR;
}

// part 2: one H2D copy of what the sorter will see into the context's text buffer
static int stage_host_h2d(BlockJob& J, bscgpu_ctx* c)
{
    J.c = c; J.dInput = c->dL;
    if (hipSetDevice(c->device) != hipSuccess) return LIBBSC_GPU_ERROR;
    if (J.dev_lzp) {                                            // the raw block goes up; the stage makes the sorter's input of it
        if (hipMemcpyAsync(c->dT, J.hInput, (size_t)J.n_orig, hipMemcpyHostToDevice, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
        return stage_device_lzp(J, c);
    }
    const unsigned char* data = J.lz ? J.lz.get() : J.hInput;
    if (hipMemcpyAsync(c->dL, data, (size_t)J.n, hipMemcpyHostToDevice, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
    return LIBBSC_NO_ERROR;
}

extern "C" BSCGPU_API long long bscgpu_process_counter(int key)
{
    switch (key) {
        case BSCGPU_PCNT_DEVICE_MODEL_BLOCKS:     return (long long)g_count_devmodel.load(std::memory_order_relaxed);
        case BSCGPU_PCNT_REDONE_ON_HOST_MODEL:    return (long long)g_count_redo.load(std::memory_order_relaxed);
        case BSCGPU_PCNT_DEVICE_MODEL_LZP_BLOCKS: return (long long)g_count_devmodel_lzp.load(std::memory_order_relaxed);
        case BSCGPU_PCNT_DEVICE_LZP_BLOCKS:       return (long long)g_count_device_lzp.load(std::memory_order_relaxed);
    }
    return LIBBSC_BAD_PARAMETER;
}

// A block that took the device model but has a sub-block that does not compress (or needs the strictly serial framing) is
// run again with the model on the host: raw sub-blocks are rebuilt from the run arrays, which that path never copied.  Rare
// (such blocks are mostly caught before by their run count); the caller must be the thread that owns the context's GPU stage.
// For an LZP-preprocessed block the sorter's input is the LZP output, which is why a device-model block keeps it until here.
static int redo_on_host_model(BlockJob& J)
{
    g_count_redo.fetch_add(1, std::memory_order_relaxed);
    J.redo.store(false, std::memory_order_relaxed);
    int rc = LIBBSC_NO_ERROR;
    if (J.hInput) rc = stage_host_h2d(J, J.c);                 // (with the device's LZP stage: upload and stage again — deterministic)
    else if (J.dev_lzp) rc = stage_device_lzp(J, J.c);
    if (rc >= 0) rc = gpu_stage(J, J.sorter, false);
    J.lz.reset();
    if (rc < 0) { J.result = rc; return rc; }
    host_stage(J);
    return J.result;
}

// bsc_compress (libbsc.cpp:213-338; input == output selects the in-place rules, :83-211): optional LZP on the host, then
// the same GPU stage + host coder as the device-resident entry point.
int bsc_compress(const unsigned char* input, unsigned char* output, int n, int lzpHashSize, int lzpMinLen,
                 int blockSorter, int coder, int features)
{
    const bool inplace = (input == output);
    int mode = 0;
    int rc = make_mode(blockSorter, coder, lzpHashSize, lzpMinLen, &mode);
    if (rc != LIBBSC_NO_ERROR) return rc;
    if (!input || !output) return LIBBSC_BAD_PARAMETER;
    if (n < 0 || n > (inplace ? 2146435072 : 1073741824)) return LIBBSC_BAD_PARAMETER;
    // The reference's in-place twin takes blocks up to 2047 MiB (libbsc.cpp:124).  The device sorter is sized and tested up to the
    // format's regular maximum, 1 GiB (tests/test_gpu_compress.py: test_max_block_1gib_golden); above it this library says so
    // instead of running an arena layout nobody has ever exercised.
    if (n > 1073741824) return LIBBSC_NOT_SUPPORTED;
    if (n <= LIBBSC_HEADER_SIZE) return bsc_store(input, output, n, features);

    std::unique_ptr<BlockJob> J(new BlockJob);
    // (the default contexts are not the caller's to set options on: BSC_DEVICE_LZP as it stands at the call decides)
    const char* const dl_env = getenv("BSC_DEVICE_LZP");
    bool declined = false;
    rc = stage_host_lzp(*J, input, output, n, lzpHashSize, lzpMinLen, &blockSorter, coder, features, mode, dl_env && dl_env[0] == '1', &declined);
    if (rc < 0) return rc;
    DefaultGpuUser user(J->n, true);
    if (user.rc != LIBBSC_NO_ERROR) return user.rc;
    bscgpu_ctx* c = user.c;
    {
        std::lock_guard<std::mutex> g(user.dev->gpu_lock);      // GPU stage; concurrent callers on this device queue here
        if (hipSetDevice(c->device) != hipSuccess) return LIBBSC_GPU_ERROR;
        if (declined) ++c->cnt_lzp_declined;
        rc = ctx_ensure_slots(c, user.slot + 1);
        if (rc < 0) return rc;
        J->slot = &c->slots[user.slot];
        rc = stage_host_h2d(*J, c);
        if (rc < 0) return rc;
        rc = gpu_stage(*J, blockSorter);
        if (!J->use_ps) J->lz.reset();                          // (a device-model block may come back for a redo: redo_on_host_model)
        if (rc < 0) return rc;
    }
    host_stage(*J);                                             // host coder: overlaps the next caller's GPU stage
    if (J->redo.load(std::memory_order_relaxed)) {
        std::lock_guard<std::mutex> g(user.dev->gpu_lock);
        if (hipSetDevice(c->device) != hipSuccess) return LIBBSC_GPU_ERROR;
        return redo_on_host_model(*J);
    }
    return J->result;
}

int bsc_lzp_compress(const unsigned char* input, unsigned char* output, int n, int hashSize, int minLen, int features)
{
    if (!input || !output || n < 0 || minLen < 4 || minLen > 255 || hashSize < 10 || hashSize > 28) return LIBBSC_BAD_PARAMETER;
    return lzp_compress(input, output, n, hashSize, minLen, features);
}
int bsc_lzp_decompress(const unsigned char* input, unsigned char* output, int n, int hashSize, int minLen, int features)
{
    (void)features;
    if (!input || !output || n < 0 || minLen < 4 || minLen > 255 || hashSize < 10 || hashSize > 28) return LIBBSC_BAD_PARAMETER;
    return lzp_decompress(input, output, n, 0x7fffffff, hashSize, minLen);
}

static int prepare_job(BlockJob& J, bscgpu_ctx* c, const void* dInput, uint8_t* output, int n, int blockSorter, int coder, int features)
{
    if (!c || !dInput || !output) return LIBBSC_BAD_PARAMETER;
    int rc = make_mode(blockSorter, coder, 0, 0, &J.mode);
    if (rc != LIBBSC_NO_ERROR) return rc;
    if (n < 0 || n > c->max_n) return LIBBSC_BAD_PARAMETER;
    J.c = c; J.dInput = dInput; J.output = output; J.n = n; J.n_orig = n; J.coder = coder; J.features = features;
    J.hInput = nullptr; J.have_adler = false; J.inplace = false; J.lz.reset();
    J.dev_lzp = false; J.dRaw = nullptr;
    J.stored_small = false; J.result = 0;
    return LIBBSC_NO_ERROR;
}

int bscgpu_compress_device(bscgpu_ctx* c, const void* dInput, uint8_t* output, int n, int blockSorter, int coder, int features)
{
    const auto t_all = clk::now();
    std::unique_ptr<BlockJob> J(new BlockJob);
    int rc = prepare_job(*J, c, dInput, output, n, blockSorter, coder, features);
    if (rc < 0) return rc;
    J->slot = &c->slots[0];
    rc = gpu_stage(*J, blockSorter);
    if (rc < 0) return rc;
    const auto t0 = clk::now();
    host_stage(*J);
    if (J->redo.load(std::memory_order_relaxed)) redo_on_host_model(*J);
    c->stage_ms[3] = ms_since(t0);
    c->stage_ms[4] = ms_since(t_all);
    return J->result;
}

int bscgpu_compress_device_lzp(bscgpu_ctx* c, const void* dInput, uint8_t* output, int n, int lzpHashSize, int lzpMinLen,
                               int blockSorter, int coder, int features)
{
    if (lzpHashSize == 0 && lzpMinLen == 0) return bscgpu_compress_device(c, dInput, output, n, blockSorter, coder, features);
    const auto t_all = clk::now();
    std::unique_ptr<BlockJob> J(new BlockJob);
    int rc = prepare_job(*J, c, dInput, output, n, blockSorter, coder, features);
    if (rc < 0) return rc;
    rc = make_mode(blockSorter, coder, lzpHashSize, lzpMinLen, &J->mode);
    if (rc != LIBBSC_NO_ERROR) return rc;
    if (!device_lzp_takes(lzpHashSize)) return LIBBSC_NOT_SUPPORTED;
    J->slot = &c->slots[0];
    if (n > LIBBSC_HEADER_SIZE) {                               // (a block as small as a header is stored, LZP or not)
        if (hipSetDevice(c->device) != hipSuccess) return LIBBSC_GPU_ERROR;
        J->dev_lzp = true; J->dRaw = dInput; J->lzp_hash = lzpHashSize; J->lzp_min = lzpMinLen; J->mode_with_lzp = J->mode;
        rc = stage_device_lzp(*J, c);
        if (rc < 0) return rc;
    }
    rc = gpu_stage(*J, blockSorter);
    if (rc < 0) return rc;
    const auto t0 = clk::now();
    host_stage(*J);
    if (J->redo.load(std::memory_order_relaxed)) redo_on_host_model(*J);
    c->stage_ms[3] = ms_since(t0);
    c->stage_ms[4] = ms_since(t_all);
    return J->result;
}

// CPUs this process can actually use: min(affinity mask, cgroup v2 cpu.max quota), clamped to [4, 64].  The coder pool of a
// pipe defaults to this (a multi-rank driver divides it between its ranks through BSCGPU_HOST_THREADS).
// CPUs of CPU time the cgroup grants (cgroup v2 cpu.max), 0 if unlimited or unknown
static int cgroup_quota_cpus()
{
    int c = 0;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[64]; long long period = 0;
        if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
            const long long quota = atoll(q);
            if (quota > 0) c = (int)(quota / period);
        }
        fclose(f);
    }
    return c;
}
static int default_coder_threads()
{
    int n = (int)std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0) n = c; }
    { const int c = cgroup_quota_cpus(); if (c >= 1 && c < n) n = c; }
    if (n < 4) n = 4;
    if (n > 64) n = 64;
    return n;
}

// Where the pool's threads may run (round 6, profiles/r06/pool_affinity.txt).  The 1-GPU boxes grant 16 CPUs of CPU TIME on a machine of
// 2 x 64 cores x 2 hardware threads, and leave the process free to run anywhere: coder threads then share cores with their SMT siblings
// and read a landing zone on the other socket whenever the scheduler says so.  Kept to one hardware thread per core of the GPU's own NUMA
// node a 20-block job runs 4472 MB/s against 4228 left alone (means of five interleaved runs, spread 4286-4663 against 3980-4553);
// long jobs are level.  Rule: of the CPUs the process may use, the first hardware thread of every core — on the GPU's node when the
// process sees ONE GPU (several GPUs: all nodes) — provided the machine is NOT meant to be filled: the cgroup grants a quota of CPU time
// and the whole quota fits on the chosen CPUs (every process of the cgroup can then follow the same rule: eight ranks of a node share
// one quota).  Without a quota the hardware threads are all the process's to use, and nothing is restricted.
// BSCGPU_HOST_AFFINITY=0 turns it off, =<cpu list> (e.g. 0-31,64-95) sets it by hand.
static bool parse_cpu_list(const char* t, cpu_set_t* out)
{
    CPU_ZERO(out);
    int n = 0;
    while (*t) {
        char* end = nullptr;
        const long a = strtol(t, &end, 10);
        if (end == t || a < 0 || a >= CPU_SETSIZE) return false;
        long b = a;
        if (*end == '-') { t = end + 1; b = strtol(t, &end, 10); if (end == t || b < a || b >= CPU_SETSIZE) return false; }
        for (long c = a; c <= b; ++c) { CPU_SET((int)c, out); ++n; }
        t = (*end == ',') ? end + 1 : end;
        if (*end != ',' && *end != 0 && *end != '\n') return false;
        if (*end == '\n') break;
    }
    return n > 0;
}
static bool read_cpu_list_file(const char* path, cpu_set_t* out)
{
    FILE* f = fopen(path, "r");
    if (!f) return false;
    char buf[4096]; const bool got = fgets(buf, sizeof buf, f) != nullptr;
    fclose(f);
    return got && parse_cpu_list(buf, out);
}
static bool pool_cpu_set(int budget, int device, cpu_set_t* out)
{
    const char* e = getenv("BSCGPU_HOST_AFFINITY");
    if (e && e[0] == '0' && e[1] == 0) return false;
    if (e && e[0] && !(e[0] == '1' && e[1] == 0)) return parse_cpu_list(e, out);
    const int quota = cgroup_quota_cpus();
    if (quota <= 0) return false;                                       // no CPU-time limit: every hardware thread is there to be used
    cpu_set_t allowed;
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return false;
    // the GPU's NUMA node, if the process sees exactly one GPU
    cpu_set_t node; bool have_node = false;
    int ndev = 0;
    if (device >= 0 && hipGetDeviceCount(&ndev) == hipSuccess && ndev == 1) {
        char bus[64];
        if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) == hipSuccess) {
            for (char* q = bus; *q; ++q) if (*q >= 'A' && *q <= 'F') *q = (char)(*q - 'A' + 'a');
            char path[160]; snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
            int nd = -1;
            if (FILE* f = fopen(path, "r")) { if (fscanf(f, "%d", &nd) != 1) nd = -1; fclose(f); }
            if (nd >= 0) { snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", nd); have_node = read_cpu_list_file(path, &node); }
        }
    } else (void)hipGetLastError();
    for (int pass = have_node ? 0 : 1; pass < 2; ++pass) {              // pass 0: the GPU's node only; pass 1: every node
        CPU_ZERO(out);
        int n = 0;
        for (int c = 0; c < CPU_SETSIZE; ++c) {
            if (!CPU_ISSET(c, &allowed) || (pass == 0 && !CPU_ISSET(c, &node))) continue;
            char path[128]; snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", c);
            cpu_set_t sib;
            if (!read_cpu_list_file(path, &sib)) return false;           // no topology: leave the threads alone
            int first = -1;
            for (int k = 0; k < CPU_SETSIZE; ++k) if (CPU_ISSET(k, &sib) && CPU_ISSET(k, &allowed)) { first = k; break; }
            if (first == c) { CPU_SET(c, out); ++n; }
        }
        if (n >= budget && n >= quota && n < CPU_COUNT(&allowed)) return true;        // (n == allowed: nothing to restrict)
    }
    return false;
}

// Optional task trace (BSCGPU_POOL_TRACE=1; bench.py BSC_BENCH_TRACE prints it): when each coder task ran — the only way to see where a
// short job's drain goes, since a pipe's caller learns of a finished block only when it next asks.
struct PoolTraceRec { double t0, t1; const void* job; int sub, shape, features; };
static std::mutex g_trace_mu;
static std::vector<PoolTraceRec> g_trace;
static const bool g_trace_on = [] { const char* e = getenv("BSCGPU_POOL_TRACE"); return e && e[0] == '1'; }();
static double trace_now() { return std::chrono::duration<double>(clk::now().time_since_epoch()).count(); }
extern "C" BSCGPU_API int bscgpu_coder_pool_trace(double* out /* [cap][6]: start, end (seconds, steady clock), job id, sub-block, sub-blocks per task, features */, int cap, int reset)
{
    std::lock_guard<std::mutex> g(g_trace_mu);
    int n = 0;
    for (const PoolTraceRec& r : g_trace) {
        if (n >= cap) break;
        out[6 * n + 0] = r.t0; out[6 * n + 1] = r.t1; out[6 * n + 2] = (double)(uintptr_t)r.job; out[6 * n + 3] = r.sub; out[6 * n + 4] = r.shape; out[6 * n + 5] = r.features;
        ++n;
    }
    if (reset) g_trace.clear();
    return n;
}
extern "C" BSCGPU_API double bscgpu_steady_now() { return trace_now(); }

// ---- pipe: several blocks in flight -------------------------------------------------------------------------
// submit() runs the GPU stage on the calling thread and queues the block's host work as tasks for the coder pool: ONE pool per
// process (the CPUs it may use: affinity and cgroup quota, default_coder_threads(); BSCGPU_HOST_THREADS overrides the number of
// threads, BSCGPU_HOST_CPUS the CPU budget the idle test below counts against — a multi-rank driver gives each rank its share),
// shared by every pipe — several contexts per GPU, as bench.py runs them, draw on the same threads, so a block whose own pipe
// is momentarily quiet is coded by whoever is free, and the pool knows how busy the process's CPUs are (ps_group).  FIFO; the
// worker that finishes a block's last task frames it.
struct CoderPool {
    struct Task { BlockJob* job; int sub; };          // sub = -1: whole host stage of the block as one task; else first sub-block of the task
    std::mutex mu; std::condition_variable cv_work, cv_done;
    std::deque<Task> queue;
    std::vector<std::thread> workers;
    int active = 0, budget = 0, users = 0;
    long long to_come = -1;                           // blocks of the announced job not yet queued (bscgpu_coder_pool_expect); -1: none announced
    int to_come_gpus = 1;
    bool stop = false;

    void worker_loop()
    {
        for (;;) {
            Task t;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_work.wait(lk, [&] { return stop || !queue.empty(); });
                if (queue.empty()) return;
                t = queue.front(); queue.pop_front();
                ++active;
            }
            BlockJob& J = *t.job;
            bool finished = false;
            const double tr0 = g_trace_on ? trace_now() : 0.0;
            const int tr_shape = J.use_ps ? J.ps_g : 0, tr_feat = J.features;
            if (t.sub == -1) { host_stage(J); finished = true; }
            else {
                if (J.use_ps) host_encode_group(J, t.sub); else host_encode_sub(J, t.sub);
                if (J.remaining.fetch_sub(1, std::memory_order_acq_rel) == 1) { host_finalize(J); finished = true; }
            }
            if (g_trace_on) { const double tr1 = trace_now(); std::lock_guard<std::mutex> g(g_trace_mu); g_trace.push_back({tr0, tr1, (const void*)&J, t.sub, tr_shape, tr_feat}); }
            { std::lock_guard<std::mutex> lk(mu); --active; if (finished) J.done = true; }
            if (finished) cv_done.notify_all();
        }
    }
    // CPUs of the budget that have neither a task nor one waiting for them (caller holds mu)
    int free_cpus() const { const int f = budget - active - (int)queue.size(); return f < 0 ? 0 : f; }
};
static std::mutex g_pool_mu;
static CoderPool* g_pool = nullptr;

static std::atomic<uint64_t> g_pool_mode[4];          // blocks queued as: 8 scalar tasks, 4 pair tasks, one eight-lane task, host-model tasks

// The caller's knowledge of where a job ENDS: `blocks` more blocks will be submitted to this process's pipes (any of them); the pool then
// shapes the host tasks of the blocks whose GPU stages end last for latency (ps_group).  blocks < 0: no announcement (the default).
static long long g_pending_expect = -1; static int g_pending_gpus = 1;      // an announcement made before the first pipe exists (under g_pool_mu)
extern "C" BSCGPU_API int bscgpu_coder_pool_expect(long long blocks, int gpus)
{
    if (gpus < 1) gpus = 1;
    std::lock_guard<std::mutex> g(g_pool_mu);
    if (!g_pool) { g_pending_expect = blocks < 0 ? -1 : blocks; g_pending_gpus = gpus; return LIBBSC_NO_ERROR; }
    std::lock_guard<std::mutex> lk(g_pool->mu);
    g_pool->to_come = blocks < 0 ? -1 : blocks;
    g_pool->to_come_gpus = gpus;
    return LIBBSC_NO_ERROR;
}

void bscgpu_coder_pool_stats(uint64_t out[4], int reset)
{
    for (int i = 0; i < 4; ++i) { out[i] = g_pool_mode[i].load(std::memory_order_relaxed); if (reset) g_pool_mode[i].store(0, std::memory_order_relaxed); }
}

static CoderPool* pool_acquire(int device = -1)
{
    std::lock_guard<std::mutex> g(g_pool_mu);
    if (!g_pool) {
        CtxTimer tm("coder pool threads");
        CoderPool* P = new CoderPool;
        // A quarter more threads than CPUs (round 5: the library's default; bench.py had been asking for half as many again since round
        // 3): a task spends part of its life asleep, waiting for its sub-blocks' copy from the GPU, so some surplus pays — but where the
        // CPUs are a cgroup QUOTA (CPU time, not cores: the 1-GPU boxes grant 16 of 256 hardware threads), 24 runnable threads at the tail of
        // a job overdraw it and the whole process, GPU-driving threads included, is stopped for the rest of the 100 ms period
        // (cpu.stat: one throttled period per 20-step run with 24 threads, none with 20; 3802 / 3844 MB/s against 4015 / 3941, 16
        // threads 3693 / 3701, one box, alternating runs, profiles/r05/coder_threads_and_quota.txt).  A cap on the tasks CODING at the same
        // time (budget - 1 slots, taken after a task's input has landed) was built and measured as well: no gain at 20 or 28 threads
        // (3565 against 3690 MB/s, means of three alternating runs, profiles/r05/coding_slots_and_tail_marks.txt) — removed.
        const int cpus = default_coder_threads();
        int nworkers = cpus + cpus / 4; if (nworkers > 96) nworkers = 96;
        bool forced = false;
        if (const char* e = getenv("BSCGPU_HOST_THREADS")) { int v = atoi(e); if (v >= 1 && v <= 256) { nworkers = v; forced = true; } }
        P->budget = (forced && nworkers < cpus) ? nworkers : cpus;
        if (const char* e = getenv("BSCGPU_HOST_CPUS")) { int v = atoi(e); if (v >= 1 && v <= 256) P->budget = v; }
        for (int i = 0; i < nworkers; ++i) P->workers.emplace_back([P] { P->worker_loop(); });
        cpu_set_t where;
        if (pool_cpu_set(P->budget, device, &where))
            for (auto& t : P->workers) (void)pthread_setaffinity_np(t.native_handle(), sizeof where, &where);
        P->to_come = g_pending_expect; P->to_come_gpus = g_pending_gpus; g_pending_expect = -1;
        g_pool = P;
    }
    ++g_pool->users;
    return g_pool;
}
static void pool_release(CoderPool* P)                 // the last pipe takes the threads with it
{
    std::unique_lock<std::mutex> g(g_pool_mu);
    if (--P->users > 0) return;
    g_pool = nullptr;
    g.unlock();
    { std::lock_guard<std::mutex> lk(P->mu); P->stop = true; }
    P->cv_work.notify_all();
    for (auto& t : P->workers) t.join();
    delete P;
}

struct bscgpu_pipe {
    bscgpu_ctx* c = nullptr;
    int depth = 1;
    int next_ticket = 0;
    struct Lane { std::unique_ptr<BlockJob> job; int ticket = -1; bool busy = false; bool joined = true; };   // ticket / joined / job->done: under the pool's mutex
    Lane lanes[MAX_SLOTS];
    CoderPool* pool = nullptr;
};

static void lane_join(bscgpu_pipe* p, bscgpu_pipe::Lane& L)
{
    if (!L.busy) return;
    {
        std::unique_lock<std::mutex> lk(p->pool->mu);
        p->pool->cv_done.wait(lk, [&] { return L.job->done; });
        L.joined = true;                            // (bscgpu_pipe_peek: from here on the lane may be reused; a peeker goes back to its caller's own bookkeeping)
    }
    p->pool->cv_done.notify_all();
    L.busy = false;
    // lane_join only runs on the pipe's submitting thread (submit / wait / destroy), which owns the GPU stage
    // (a redo that cannot be run must not leave the stale result of a block whose output was never written)
    if (L.job->redo.load(std::memory_order_relaxed)) {
        if (hipSetDevice(p->c->device) == hipSuccess) redo_on_host_model(*L.job);
        else L.job->result = LIBBSC_GPU_ERROR;
    }
    L.job->lz.reset();                              // a device-model block kept its LZP output for that redo only: a lane must not sit on a block-sized buffer until its next block
}

int bscgpu_pipe_create(bscgpu_ctx* c, int depth, bscgpu_pipe** out)
{
    if (!c || !out || depth < 1 || depth > MAX_SLOTS) return LIBBSC_BAD_PARAMETER;
    if (hipSetDevice(c->device) != hipSuccess) return LIBBSC_GPU_ERROR;
    int rc = ctx_ensure_slots(c, depth);
    if (rc < 0) return rc;
    bscgpu_pipe* p = new bscgpu_pipe;
    p->c = c; p->depth = depth;
    for (int i = 0; i < depth; ++i) p->lanes[i].job.reset(new BlockJob);
    p->pool = pool_acquire(c->device);
    *out = p;
    return LIBBSC_NO_ERROR;
}

void bscgpu_pipe_destroy(bscgpu_pipe* p)
{
    if (!p) return;
    for (int i = 0; i < p->depth; ++i) lane_join(p, p->lanes[i]);
    pool_release(p->pool);
    delete p;
}

// queue the host half of a block whose GPU stage has run
static int pipe_enqueue(bscgpu_pipe* p, bscgpu_pipe::Lane& L, int ticket)
{
    BlockJob& J = *L.job;
    L.busy = true;
    J.pipelined = p->depth >= 3;
    CoderPool* P = p->pool;
    J.pipe_workers = (int)P->workers.size();
    {
        std::lock_guard<std::mutex> lk(P->mu);
        L.ticket = ticket; L.joined = false;
        J.tail_r = -1;
        J.tail_gpus = P->to_come_gpus;
        J.tail_pipes = P->users / (P->to_come_gpus > 0 ? P->to_come_gpus : 1);
        if (P->to_come > 0) J.tail_r = (int)(--P->to_come < 0x7fffffff ? P->to_come : 0x7fffffff);
        else if (P->to_come == 0) P->to_come = -1;               // more blocks than announced: the rule is dropped
        J.done = false;                                          // (with the other fields a peeker reads, under the pool's mutex)
        p->next_ticket = ticket + 1;
        J.pool_free = P->free_cpus();
        if (job_uses_tasks(J)) {
            host_prepare(J);
            if (J.use_ps) {                                      // device model: 1 (scalar), 2 (interleaved scalar) or 8 (SIMD lanes) sub-blocks per task
                const int g = J.ps_g = ps_group(J);
                g_pool_mode[g == 1 ? 0 : g == 2 ? 1 : 2].fetch_add(1, std::memory_order_relaxed);
                J.remaining.store(J.nblocks / g, std::memory_order_release);
                for (int b = 0; b < J.nblocks; b += g) P->queue.push_back({&J, b});
            } else {
                g_pool_mode[3].fetch_add(1, std::memory_order_relaxed);
                J.remaining.store(J.nblocks, std::memory_order_release);
                for (int b = 0; b < J.nblocks; ++b) P->queue.push_back({&J, b});
            }
        } else {
            g_pool_mode[3].fetch_add(1, std::memory_order_relaxed);
            P->queue.push_back({&J, -1});
        }
    }
    P->cv_work.notify_all();
    return ticket;
}

int bscgpu_pipe_submit(bscgpu_pipe* p, const void* dInput, uint8_t* output, int n, int blockSorter, int coder, int features)
{
    if (!p) return LIBBSC_BAD_PARAMETER;
    const int ticket = p->next_ticket;
    bscgpu_pipe::Lane& L = p->lanes[ticket % p->depth];
    lane_join(p, L);                                // the slot's previous block must be finished before its buffers are reused
    BlockJob& J = *L.job;
    int rc = prepare_job(J, p->c, dInput, output, n, blockSorter, coder, features);
    if (rc < 0) return rc;
    J.slot = &p->c->slots[ticket % p->depth];
    rc = gpu_stage(J, blockSorter);
    J.lz.reset();                                   // (device-resident input: there is no LZP output)
    if (rc < 0) return rc;
    return pipe_enqueue(p, L, ticket);
}

// Host-resident block with the full bsc_compress parameter set (LZP included); `input` must stay valid until the
// ticket has been waited for (a block that does not compress is stored from it).
int bscgpu_pipe_submit_host(bscgpu_pipe* p, const uint8_t* input, uint8_t* output, int n, int lzpHashSize, int lzpMinLen,
                            int blockSorter, int coder, int features)
{
    if (!p || !input || !output) return LIBBSC_BAD_PARAMETER;
    int mode = 0;
    int rc = make_mode(blockSorter, coder, lzpHashSize, lzpMinLen, &mode);
    if (rc != LIBBSC_NO_ERROR) return rc;
    if (n < 0 || n > p->c->max_n) return LIBBSC_BAD_PARAMETER;
    const int ticket = p->next_ticket;
    bscgpu_pipe::Lane& L = p->lanes[ticket % p->depth];
    lane_join(p, L);
    BlockJob& J = *L.job;
    J.slot = &p->c->slots[ticket % p->depth];
    if (n <= LIBBSC_HEADER_SIZE) {
        J.c = p->c; J.n = J.n_orig = n; J.output = output; J.lz.reset();
        J.result = bsc_store(input, output, n, features);
        J.stored_small = true;
        return pipe_enqueue(p, L, ticket);
    }
    bool declined = false;
    rc = stage_host_lzp(J, input, output, n, lzpHashSize, lzpMinLen, &blockSorter, coder, features, mode, p->c->device_lzp != 0, &declined);
    if (rc < 0) return rc;
    if (declined) ++p->c->cnt_lzp_declined;
    rc = stage_host_h2d(J, p->c);
    if (rc < 0) return rc;
    rc = gpu_stage(J, blockSorter);
    if (!J.use_ps) J.lz.reset();                    // the LZP output lives in HBM from here on; a device-model block keeps it for a possible redo
    if (rc < 0) return rc;
    return pipe_enqueue(p, L, ticket);
}

// Any thread: block until the HOST stage of `ticket` has finished and, if the block is then complete, hand out its result — without
// retiring the ticket (bscgpu_pipe_wait on the submitting thread still does that).  Returns 1 with *result set; 0 when the block needs
// its submitting thread after all (a redo on the host model runs the GPU stage again) or the ticket has already been retired / its
// lane reused; a negative code for bad arguments.  For collectors that take blocks in order while the submitting thread is busy
// with the GPU stages of later blocks (job.cpp): a finished block's output buffer is final from here on.
int bscgpu_pipe_peek(bscgpu_pipe* p, int ticket, int* result)
{
    if (!p || !result || ticket < 0) return LIBBSC_BAD_PARAMETER;
    bscgpu_pipe::Lane& L = p->lanes[ticket % p->depth];
    std::unique_lock<std::mutex> lk(p->pool->mu);
    if (ticket >= p->next_ticket) return LIBBSC_BAD_PARAMETER;       // not submitted (yet): nothing to wait for
    p->pool->cv_done.wait(lk, [&] { return L.ticket != ticket || L.joined || L.job->done; });
    if (L.ticket != ticket || L.joined) return 0;
    if (L.job->redo.load(std::memory_order_relaxed)) return 0;
    *result = L.job->result;
    return 1;
}

int bscgpu_pipe_wait(bscgpu_pipe* p, int ticket)
{
    if (!p || ticket < 0 || ticket >= p->next_ticket) return LIBBSC_BAD_PARAMETER;
    bscgpu_pipe::Lane& L = p->lanes[ticket % p->depth];
    if (L.ticket != ticket) return LIBBSC_BAD_PARAMETER;   // already overwritten by a later submit
    lane_join(p, L);
    return L.job->result;
}

// ---- `synth-text v1` -----------------------------------------------------------------
int bsc_synth_text_v1(unsigned long long seed, unsigned char* out, long long n)
{
    if (seed == 0 || !out || n < 0) return LIBBSC_BAD_PARAMETER;
    unsigned long long s = seed;
    auto next = [&]() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 2685821657736338717ull; };
    static thread_local unsigned char vocab[4096][10];
    static thread_local unsigned char vlen[4096];
    for (int w = 0; w < 4096; ++w) {
        const int len = 2 + (int)(next() % 8);
        vlen[w] = (unsigned char)len;
        for (int i = 0; i < len; ++i) vocab[w][i] = (unsigned char)('a' + next() % 26);
    }
    long long pos = 0, words = 0;
    while (pos < n) {
        const unsigned long long r = next();
        const unsigned idx = (unsigned)(((r & 0xfff) * ((r >> 12) & 0xfff)) >> 12);
        for (int i = 0; i < vlen[idx] && pos < n; ++i) out[pos++] = vocab[idx][i];
        ++words;
        if (pos < n) out[pos++] = (words % 16 == 0) ? '\n' : ' ';
    }
    return LIBBSC_NO_ERROR;
}

}  // extern "C"

// ---- batched compression of many small blocks (bscgpu_*_batch, include/bscgpu.h) ------------------------------------------------
// Blocks below BSCGPU_BATCH_MAX_N that the BWT sorts go through one suffix sort per PASS (bwt.hip: bwt_batch_device), the
// blocks that ST3..ST8 sort through one sort transform per pass (st.hip: st_batch_device, bscgpu_st_batch_plan), the
// rest through the single-block path on the same context.  After a pass's sort its L comes back in one copy and every block is coded
// on the host exactly as bsc_compress codes it (libbsc.cpp:283-337: bsc_coder_compress, the stored rule, the trailer); that coding
// overlaps the next pass's sort.

extern "C" BSCGPU_API int bscgpu_batch_plan(const int* sizes, int count, int blockSorter, int64_t cap, int* pass_of)
{
    if (count < 0 || (count > 0 && (!sizes || !pass_of))) return LIBBSC_BAD_PARAMETER;
    return batch_pass_plan_bwt(sizes, count, blockSorter, cap, pass_of);
}

// The same rule for the sort transform: blocks of 1 .. BSCGPU_ST_BATCH_MAX_N - 1 bytes ride in passes (a block of one byte too: its
// record sorts like any other), an empty block is an empty entry of a pass's table, every k has the same block cap.
extern "C" BSCGPU_API int bscgpu_st_batch_plan(const int* sizes, int count, int k, int64_t cap, int* pass_of)
{
    if (count < 0 || (count > 0 && (!sizes || !pass_of)) || k < LIBBSC_BLOCKSORTER_ST3 || k > LIBBSC_BLOCKSORTER_ST8) return LIBBSC_BAD_PARAMETER;
    for (int b = 0; b < count; ++b) if (sizes[b] < 0) return LIBBSC_BAD_PARAMETER;
    return batch_pass_plan_st(sizes, count, cap, pass_of);
}

static int plan_for(const int* sizes, int count, int blockSorter, int64_t cap, int* pass_of)
{
    if (blockSorter >= LIBBSC_BLOCKSORTER_ST3 && blockSorter <= LIBBSC_BLOCKSORTER_ST8) return bscgpu_st_batch_plan(sizes, count, blockSorter, cap, pass_of);
    return bscgpu_batch_plan(sizes, count, blockSorter, cap, pass_of);
}

extern "C" BSCGPU_API int bscgpu_st_batch_device(bscgpu_ctx* c, const void* dT, void* dOut, const int* sizes, int count, int k, int* index)
{
    if (!c || count < 0 || (count > 0 && (!sizes || !index)) || k < LIBBSC_BLOCKSORTER_ST3 || k > LIBBSC_BLOCKSORTER_ST8) return LIBBSC_BAD_PARAMETER;
    int64_t total = 0;
    for (int b = 0; b < count; ++b) { if (sizes[b] < 0) return LIBBSC_BAD_PARAMETER; total += sizes[b]; }
    if (total > 0 && (!dT || !dOut)) return LIBBSC_BAD_PARAMETER;
    if (count == 0) return LIBBSC_NO_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return LIBBSC_GPU_ERROR;
    std::vector<int> pass_of((size_t)count);
    const int npass = bscgpu_st_batch_plan(sizes, count, k, c->max_n, pass_of.data());
    if (npass < 0) return npass;
    std::vector<int64_t> off((size_t)count + 1, 0);
    for (int b = 0; b < count; ++b) off[b + 1] = off[b] + sizes[b];
    const u8* T = (const u8*)dT; u8* O = (u8*)dOut;
    for (int b = 0; b < count;) {
        if (pass_of[b] < 0) {                        // alone: what bscgpu_st_encode_device gives (a block above max_n: its error code)
            index[b] = 0;
            if (sizes[b] > 0) { const int rc = st_device(c, T + off[b], O + off[b], sizes[b], k, &index[b]); if (rc < 0) index[b] = rc; }
            ++b;
            continue;
        }
        const int e = batch_pass_end(pass_of.data(), sizes, count, b);
        const int rc = st_batch_device(c, T + off[b], O + off[b], sizes + b, e - b, k, nullptr, index + b);
        if (rc < 0) return rc;
        b = e;
    }
    return LIBBSC_NO_ERROR;
}

extern "C" BSCGPU_API int bscgpu_bwt_batch_device(bscgpu_ctx* c, const void* dT, void* dL, const int* sizes, int count, int* primary,
                                                  unsigned char* num_indexes, int* indexes)
{
    if (!c || count < 0 || (count > 0 && (!sizes || !primary)) || (num_indexes != nullptr && indexes == nullptr)) return LIBBSC_BAD_PARAMETER;
    int64_t total = 0;
    for (int b = 0; b < count; ++b) { if (sizes[b] < 0) return LIBBSC_BAD_PARAMETER; total += sizes[b]; }
    if (total > 0 && (!dT || !dL)) return LIBBSC_BAD_PARAMETER;
    if (count == 0) return LIBBSC_NO_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return LIBBSC_GPU_ERROR;
    const bool aux = num_indexes != nullptr;
    std::vector<int> pass_of((size_t)count), rate((size_t)count);
    const int npass = bscgpu_batch_plan(sizes, count, LIBBSC_BLOCKSORTER_BWT, c->max_n, pass_of.data());
    if (npass < 0) return npass;
    std::vector<int64_t> off((size_t)count + 1, 0);
    for (int b = 0; b < count; ++b) off[b + 1] = off[b] + sizes[b];
    // what bsc_bwt_encode says before sorting anything (n = 0; r < 2 with the indexes asked for)
    for (int b = 0; b < count; ++b) {
        const int n = sizes[b];
        if (aux) num_indexes[b] = 0;
        rate[b] = aux ? aux_rate(n) : 0;
        if (n == 0) { primary[b] = aux ? LIBBSC_BAD_PARAMETER : 0; rate[b] = -1; }
        else if (aux && rate[b] < 2) { primary[b] = LIBBSC_BAD_PARAMETER; rate[b] = -1; }
    }
    const u8* T = (const u8*)dT; u8* L = (u8*)dL;
    auto put = [&](int b, const uint32_t* I) {
        primary[b] = (int)I[0];
        if (aux) {
            const int cnt = (sizes[b] - 1) / rate[b];
            num_indexes[b] = (unsigned char)cnt;
            for (int t = 0; t < cnt; ++t) indexes[16 * b + t] = (int)I[t + 1] - 1;
        }
    };
    std::vector<uint32_t> res((size_t)BATCH_MAX_BLOCKS * 16);
    for (int b = 0; b < count;) {
        if (pass_of[b] < 0) {
            if (sizes[b] > 0 && rate[b] >= 0) {
                uint32_t I[256]; int64_t p = 0;
                const int rc = bwt_device(c, T + off[b], L + off[b], sizes[b], rate[b], aux ? I : nullptr, &p);
                if (rc < 0) primary[b] = rc;
                else if (aux) put(b, I);
                else primary[b] = (int)p;
            } else if (sizes[b] > 0 && L + off[b] != T + off[b]) {
                if (hipMemcpyAsync(L + off[b], T + off[b], (size_t)sizes[b], hipMemcpyDeviceToDevice, c->stream) != hipSuccess || ctx_sync(c) != hipSuccess) return LIBBSC_GPU_ERROR;
            }
            ++b;
            continue;
        }
        const int e = batch_pass_end(pass_of.data(), sizes, count, b);      // the pass: one contiguous range
        const int rc = bwt_batch_device(c, T + off[b], L + off[b], sizes + b, e - b, rate.data() + b, res.data());
        if (rc < 0) return rc;
        for (int q = b; q < e; ++q) if (rate[q] >= 0 && sizes[q] > 0) put(q, res.data() + 16 * (size_t)(q - b));
        b = e;
    }
    return LIBBSC_NO_ERROR;
}

// bsc_compress on a given context (the body of bsc_compress without the default-context lookup)
static int compress_one_on_ctx(bscgpu_ctx* c, const unsigned char* input, unsigned char* output, int n, int lzpHashSize, int lzpMinLen,
                               int blockSorter, int coder, int features)
{
    int mode = 0;
    int rc = make_mode(blockSorter, coder, lzpHashSize, lzpMinLen, &mode);
    if (rc != LIBBSC_NO_ERROR) return rc;
    if (n < 0 || n > 1073741824) return LIBBSC_BAD_PARAMETER;
    if (n <= LIBBSC_HEADER_SIZE) return bsc_store(input, output, n, features);
    if (n > c->max_n) return LIBBSC_GPU_NOT_ENOUGH_MEMORY;        // (the call's context is not resized: bscgpu.h)
    std::unique_ptr<BlockJob> J(new BlockJob);
    bool declined = false;
    rc = stage_host_lzp(*J, input, output, n, lzpHashSize, lzpMinLen, &blockSorter, coder, features, mode, c->device_lzp != 0, &declined);
    if (rc < 0) return rc;
    if (declined) ++c->cnt_lzp_declined;
    if (J->n > c->max_n) return LIBBSC_GPU_NOT_ENOUGH_MEMORY;
    if (hipSetDevice(c->device) != hipSuccess) return LIBBSC_GPU_ERROR;
    rc = ctx_ensure_slots(c, 1);
    if (rc < 0) return rc;
    J->slot = &c->slots[0];
    rc = stage_host_h2d(*J, c);
    if (rc < 0) return rc;
    rc = gpu_stage(*J, blockSorter);
    if (!J->use_ps) J->lz.reset();
    if (rc < 0) return rc;
    host_stage(*J);
    if (J->redo.load(std::memory_order_relaxed)) return redo_on_host_model(*J);
    return J->result;
}

static_assert(BATCH_PASS_MAX_BLOCKS == BATCH_MAX_BLOCKS, "batch_pass_plan.h plans passes of as many blocks as the sorters take");

namespace {
struct BatchBlock {
    int b = 0, lz = 0, mode = 0, index = 0, num_indexes = 0;
    int indexes[16];
    unsigned adler = 0;                          // Adler-32 of the block's input (device input: from the pass's segmented kernel)
    BatchClass cls = BATCH_EMPTY;                // what became of it in the pass's preparation (batch_pass_plan.h)
    unsigned char* lzbuf = nullptr;
};

// What a block of a sorted pass is coded from (batch_pass_plan.h: batch_block_source): its L, or entry li of the pass's front-end layout
// with its run arrays, the pass's probability stream from the device model of this coder (ps, sub-block s at poff[s]; packed: the
// BSCGPU_RC_STATIC13 bodies at pbase[s]) or the sub-blocks as the device's range coder left them (BSCGPU_OPT_DEVICE_RC: rc_res[s] bytes,
// or LIBBSC_NOT_COMPRESSIBLE, at rc_bytes + rc_off[s], coded with a budget of rc_room[s]; see front_batch_code_rc)
struct PassSource {
    BatchSource kind;
    const unsigned char* L;
    const bscgpu_front_layout* lay; int li;
    const uint16_t* ps; const uint32_t* poff; const int64_t* pbase;
    const uint8_t* rc_bytes; const uint32_t* rc_off; const int* rc_res; const int* rc_room;
    bool packed;         // (the coded streams were BSCGPU_RC_STATIC13 bodies, whose LIBBSC_NOT_COMPRESSIBLE is not the reference's)
};
}

static int front_batch_code_rc(const bscgpu_front_layout* Lo, int block, const uint8_t* bytes, const uint32_t* off, const int* res, const int* room_of,
                               unsigned char* out, int coder, int features, bool packed);

// the coder's part of it -> the bytes in out, or a negative code
static int code_from_source(const PassSource& S, int lz, unsigned char* out, int coder, int features)
{
    switch (S.kind) {
    case BATCH_FROM_L:         return coder_compress(S.L, out, lz, coder, features);
    case BATCH_FROM_RUNS:      return bscgpu_front_batch_code(S.lay, S.li, out, coder, features);
    case BATCH_FROM_PS16:      return bscgpu_front_batch_code_ps(S.lay, S.li, S.ps, S.poff, out, features);
    case BATCH_FROM_PS13:      return bscgpu_front_batch_code_ps13(S.lay, S.li, reinterpret_cast<const uint8_t*>(S.ps), S.poff, S.pbase, out, features);
    case BATCH_FROM_FAST:      return bscgpu_front_batch_code_psf(S.lay, S.li, S.ps, S.poff, out, features);
    case BATCH_FROM_DEVICE_RC: return front_batch_code_rc(S.lay, S.li, S.rc_bytes, S.rc_off, S.rc_res, S.rc_room, out, coder, features, S.packed);
    }
    return LIBBSC_BAD_PARAMETER;
}

// the host tail of bsc_compress (libbsc.cpp:296-336) for one block of a sorted pass; input: host bytes, or dIn in HBM
static int code_sorted_block(bscgpu_ctx* c, const unsigned char* input, const unsigned char* dIn, unsigned char* output, int n,
                             const BatchBlock& B, int coder, int features, const PassSource* src)
{
    unsigned char* buffer = (unsigned char*)bsc_malloc((size_t)B.lz + 4096);
    if (!buffer) return LIBBSC_NOT_ENOUGH_MEMORY;
    int result = code_from_source(*src, B.lz, buffer, coder, features);
    if (result >= LIBBSC_NO_ERROR) memcpy(block_body(output), buffer, (size_t)result);
    bsc_free(buffer);
    const int num = n < 64 * 1024 ? 0 : B.num_indexes;
    const unsigned adler = input ? adler32(input, (size_t)n) : B.adler;
    const int size = block_finish_coded(output, n, result, B.mode, B.index, B.indexes, num, adler);
    if (size != LIBBSC_NOT_COMPRESSIBLE) return size;
    if (!input) return store_from_device(c, dIn, output, n, adler);
    memmove(block_body(output), input, (size_t)n);         // (bsc_store, without a second pass for the checksum)
    return block_finish_stored(output, n, adler);
}

// ---- the QLFC front end of a whole pass: layout on the host, coding of one block from a layout (include/bscgpu.h) ----------------
static int front_layout_args(const int* sizes, int count, const bscgpu_front_layout* out)
{
    if (count < 0 || count > BATCH_MAX_BLOCKS || !out || (count > 0 && !sizes) || !out->blk_sub || !out->sub_run) return LIBBSC_BAD_PARAMETER;
    int64_t total = 0;
    for (int b = 0; b < count; ++b) { if (sizes[b] < 0 || sizes[b] >= BSCGPU_BATCH_MAX_N) return LIBBSC_BAD_PARAMETER; total += sizes[b]; }
    if (count > 0 && (!out->sub_start || !out->sub_size || !out->nsym || !out->first_seen)) return LIBBSC_BAD_PARAMETER;
    if (total > 0 && (!out->sym || !out->rank || !out->start)) return LIBBSC_BAD_PARAMETER;
    return LIBBSC_NO_ERROR;
}

extern "C" BSCGPU_API int bscgpu_front_batch_host(const unsigned char* L, const int* sizes, int count, bscgpu_front_layout* out)
{
    const int arc = front_layout_args(sizes, count, out);
    if (arc < 0) return arc;
    out->count = count; out->sizes = sizes;
    int nsub = 0; int64_t m = 0, off = 0;
    QlfcRuns R;
    for (int b = 0; b < count; ++b) {
        out->blk_sub[b] = nsub;
        const int n = sizes[b];
        if (n == 0) continue;
        if (!L) return LIBBSC_BAD_PARAMETER;
        const int nb = coder_num_blocks(n);
        int st[8], sz[8];
        if (nb == 1) { st[0] = 0; sz[0] = n; } else coder_split_blocks(L + off, n, nb, st, sz);
        for (int q = 0; q < nb; ++q, ++nsub) {
            qlfc_runs(L + off + st[q], sz[q], R);
            const RunView& V = R.view;
            out->sub_start[nsub] = st[q]; out->sub_size[nsub] = sz[q]; out->sub_run[nsub] = (uint32_t)m;
            out->nsym[nsub] = V.nsym;
            memcpy(out->first_seen + 256 * (size_t)nsub, V.first_seen, (size_t)V.nsym);
            memcpy(out->sym + m, V.sym, V.count); memcpy(out->rank + m, V.rank, V.count);
            for (uint32_t j = 0; j < V.count; ++j) out->start[m + j] = V.start[j] + (uint32_t)st[q];
            m += V.count;
        }
        off += n;
    }
    out->blk_sub[count] = nsub; out->sub_run[nsub] = (uint32_t)m;
    out->nsub = nsub; out->m = m;
    return LIBBSC_NO_ERROR;
}

// the run arrays of sub-block s of a layout
static RunView front_view(const bscgpu_front_layout* Lo, int s)
{
    RunView V;
    V.sym = Lo->sym + Lo->sub_run[s]; V.rank = Lo->rank + Lo->sub_run[s]; V.start = Lo->start + Lo->sub_run[s];
    V.count = Lo->sub_run[s + 1] - Lo->sub_run[s];
    V.end = (uint32_t)(Lo->sub_start[s] + Lo->sub_size[s]);
    V.nsym = Lo->nsym[s];
    memcpy(V.first_seen, Lo->first_seen + 256 * (size_t)s, (size_t)V.nsym);
    return V;
}
static void front_views(const bscgpu_front_layout* Lo, int block, RunView* views)
{
    const int s0 = Lo->blk_sub[block], nb = Lo->blk_sub[block + 1] - s0;
    for (int q = 0; q < nb; ++q) views[q] = front_view(Lo, s0 + q);
}

extern "C" BSCGPU_API int bscgpu_front_batch_code(const bscgpu_front_layout* Lo, int block, unsigned char* out, int coder, int features)
{
    if (!Lo || !out || block < 0 || block >= Lo->count) return LIBBSC_BAD_PARAMETER;
    const int s0 = Lo->blk_sub[block], nb = Lo->blk_sub[block + 1] - s0;
    if (nb < 1 || nb > 8) return LIBBSC_BAD_PARAMETER;             // (an empty block: what bsc_coder_compress says to n = 0)
    RunView views[8];
    front_views(Lo, block, views);
    RunsFetch fetch(views, Lo->sub_start + s0, Lo->sub_size + s0, nb);
    return coder_compress_views(views, nb, Lo->sub_start + s0, Lo->sub_size + s0, Lo->sizes[block], out, coder, features, fetch);
}

static int64_t pstream_host(const bscgpu_front_layout* Lo, int s, uint16_t* out, int64_t cap, int coder)
{
    if (!Lo || s < 0 || s >= Lo->nsub || cap < 0 || (cap > 0 && !out)) return LIBBSC_BAD_PARAMETER;
    const RunView V = front_view(Lo, s);
    return coder == LIBBSC_CODER_QLFC_FAST ? qlfc_fast_pstream_runs(V, out, cap) : qlfc_static_pstream_runs(V, out, cap);
}
extern "C" BSCGPU_API int64_t bscgpu_static_pstream_host(const bscgpu_front_layout* Lo, int s, uint16_t* out, int64_t cap)
{
    return pstream_host(Lo, s, out, cap, LIBBSC_CODER_QLFC_STATIC);
}
extern "C" BSCGPU_API int64_t bscgpu_fast_pstream_host(const bscgpu_front_layout* Lo, int s, uint16_t* out, int64_t cap)
{
    return pstream_host(Lo, s, out, cap, LIBBSC_CODER_QLFC_FAST);
}
// ... for the adaptive coder (-e2): entries in the static coder's form, dbg (optional) [4][cap]
extern "C" BSCGPU_API int64_t bscgpu_adaptive_pstream_host(const bscgpu_front_layout* Lo, int s, uint16_t* out, int64_t cap, uint16_t* dbg)
{
    if (!Lo || s < 0 || s >= Lo->nsub || cap < 0 || (cap > 0 && !out)) return LIBBSC_BAD_PARAMETER;
    return qlfc_adaptive_pstream_runs(front_view(Lo, s), out, cap, dbg);
}

// ... and the longest mixer chain of sub-block s, per_mixer (optional, [1896]) every mixer's decisions: the host walker's own count
extern "C" BSCGPU_API int64_t bscgpu_adaptive_longest_chain_host(const bscgpu_front_layout* Lo, int s, uint32_t* per_mixer)
{
    if (!Lo || s < 0 || s >= Lo->nsub) return LIBBSC_BAD_PARAMETER;
    return qlfc_adaptive_longest_chain_runs(front_view(Lo, s), per_mixer);
}

static int front_batch_code_stream(const bscgpu_front_layout* Lo, int block, const uint16_t* ps, const uint32_t* poff,
                                   unsigned char* out, int coder, int features)
{
    if (!Lo || !out || !ps || !poff || block < 0 || block >= Lo->count) return LIBBSC_BAD_PARAMETER;
    const int s0 = Lo->blk_sub[block], nb = Lo->blk_sub[block + 1] - s0;
    if (nb < 1 || nb > 8) return LIBBSC_BAD_PARAMETER;
    RunView views[8];
    front_views(Lo, block, views);
    RunsFetch fetch(views, Lo->sub_start + s0, Lo->sub_size + s0, nb);
    struct FromStream : SubEncode {                                 // the range coder alone: the model ran on the GPU
        const bscgpu_front_layout* Lo; int s0; const uint16_t* ps; const uint32_t* poff; int form;
        int operator()(int b, uint8_t* dst, int room) override
        {
            const int s = s0 + b;
            return qlfc_encode_pstream(form, PstreamJob{Lo->first_seen + 256 * (size_t)s, Lo->nsym[s], Lo->sub_size[s], ps + poff[s], (size_t)(poff[s + 1] - poff[s]), dst, room});
        }
    } enc;
    enc.Lo = Lo; enc.s0 = s0; enc.ps = ps; enc.poff = poff; enc.form = coder == LIBBSC_CODER_QLFC_FAST ? BSCGPU_RC_FAST16 : BSCGPU_RC_STATIC16;
    return coder_compress_views(views, nb, Lo->sub_start + s0, Lo->sub_size + s0, Lo->sizes[block], out, coder, features, fetch, &enc);
}
extern "C" BSCGPU_API int bscgpu_front_batch_code_ps(const bscgpu_front_layout* Lo, int block, const uint16_t* ps, const uint32_t* poff,
                                                     unsigned char* out, int features)
{
    return front_batch_code_stream(Lo, block, ps, poff, out, LIBBSC_CODER_QLFC_STATIC, features);
}
// ... for the fast coder (-e0): the sub-blocks' streams in the BSCGPU_RC_FAST16 form
extern "C" BSCGPU_API int bscgpu_front_batch_code_psf(const bscgpu_front_layout* Lo, int block, const uint16_t* ps, const uint32_t* poff,
                                                      unsigned char* out, int features)
{
    return front_batch_code_stream(Lo, block, ps, poff, out, LIBBSC_CODER_QLFC_FAST, features);
}

// ... from the packed 13-bit stream of a pass (BSCGPU_RC_STATIC13 bodies at pbase[s]).  That form has no run-start mark: its coder gives
// up at ANY decision once the output is full, the reference at a run start.  So LIBBSC_NOT_COMPRESSIBLE from the packed coder is not an
// answer: the sub-block is coded again by the host model from its runs, whose result — bytes or LIBBSC_NOT_COMPRESSIBLE, then stored
// raw — is the reference's own (what the large-block path does: "redone from the run arrays").
extern "C" BSCGPU_API int bscgpu_front_batch_code_ps13(const bscgpu_front_layout* Lo, int block, const uint8_t* packed, const uint32_t* poff,
                                                       const int64_t* pbase, unsigned char* out, int features)
{
    if (!Lo || !out || !packed || !poff || !pbase || block < 0 || block >= Lo->count) return LIBBSC_BAD_PARAMETER;
    const int s0 = Lo->blk_sub[block], nb = Lo->blk_sub[block + 1] - s0;
    if (nb < 1 || nb > 8) return LIBBSC_BAD_PARAMETER;
    for (int s = s0; s < s0 + nb; ++s) if (pbase[s] < 0 || (pbase[s] & 7) != 0) return LIBBSC_BAD_PARAMETER;      // a body starts on a group
    RunView views[8];
    front_views(Lo, block, views);
    RunsFetch fetch(views, Lo->sub_start + s0, Lo->sub_size + s0, nb);
    struct FromPacked : SubEncode {
        const bscgpu_front_layout* Lo; const RunView* views; int s0; const uint8_t* packed; const uint32_t* poff; const int64_t* pbase;
        int operator()(int b, uint8_t* dst, int room) override
        {
            const int s = s0 + b;
            const int r = qlfc_encode_pstream(BSCGPU_RC_STATIC13, PstreamJob{Lo->first_seen + 256 * (size_t)s, Lo->nsym[s], Lo->sub_size[s], packed + pbase[s] / 8 * 13,
                                                                             (size_t)(poff[s + 1] - poff[s]), dst, room});
            return r == LIBBSC_NOT_COMPRESSIBLE ? qlfc_encode_runs(views[b], Lo->sub_size[s], dst, room, LIBBSC_CODER_QLFC_STATIC) : r;
        }
    } enc;
    enc.Lo = Lo; enc.views = views; enc.s0 = s0; enc.packed = packed; enc.poff = poff; enc.pbase = pbase;
    return coder_compress_views(views, nb, Lo->sub_start + s0, Lo->sub_size + s0, Lo->sizes[block], out, LIBBSC_CODER_QLFC_STATIC, features, fetch, &enc);
}

// the CPU stand-in for the packed layout of a pass (include/bscgpu.h): a pure function
extern "C" BSCGPU_API int64_t bscgpu_pstream_pack13_host(const uint16_t* ps, const uint32_t* poff, int nsub, uint8_t* out, int64_t cap_bytes, int64_t* pbase)
{
    if (nsub < 0 || !poff || !pbase || cap_bytes < 0) return LIBBSC_BAD_PARAMETER;
    const int64_t bytes = dc_pack13_host(ps, poff, nsub, out, cap_bytes, pbase);
    return bytes < 0 ? LIBBSC_BAD_PARAMETER : bytes;
}

// bscgpu_front_batch_code_ps with the range coder's work already done on the device: the framing alone.  A sub-block whose budget
// under the caller's framing rule is not the one the device coded it with (the serial rule behind a sub-block stored raw) goes through
// the host model from its runs; one that ended LIBBSC_NOT_COMPRESSIBLE is stored raw, rebuilt from its runs — unless the streams were
// packed (BSCGPU_RC_STATIC13 gives up at any decision, not at a run start): then the host model codes it again and its answer decides.
static int front_batch_code_rc(const bscgpu_front_layout* Lo, int block, const uint8_t* bytes, const uint32_t* off, const int* res, const int* room_of,
                               unsigned char* out, int coder, int features, bool packed)
{
    const int s0 = Lo->blk_sub[block], nb = Lo->blk_sub[block + 1] - s0;
    if (nb < 1 || nb > 8) return LIBBSC_BAD_PARAMETER;
    RunView views[8];
    front_views(Lo, block, views);
    RunsFetch fetch(views, Lo->sub_start + s0, Lo->sub_size + s0, nb);
    struct Coded : SubEncode {
        const bscgpu_front_layout* Lo; const RunView* views; int s0; const uint8_t* bytes; const uint32_t* off; const int* res; const int* room_of; int coder; bool packed;
        int operator()(int b, uint8_t* dst, int room) override
        {
            const int s = s0 + b;
            if (room != room_of[s] || (packed && res[s] == LIBBSC_NOT_COMPRESSIBLE)) return qlfc_encode_runs(views[b], Lo->sub_size[s], dst, room, coder);
            if (res[s] >= 0) memcpy(dst, bytes + off[s], (size_t)res[s]);
            return res[s];
        }
    } enc;
    enc.Lo = Lo; enc.views = views; enc.s0 = s0; enc.bytes = bytes; enc.off = off; enc.res = res; enc.room_of = room_of; enc.coder = coder; enc.packed = packed;
    return coder_compress_views(views, nb, Lo->sub_start + s0, Lo->sub_size + s0, Lo->sizes[block], out, coder, features, fetch, &enc);
}

extern "C" BSCGPU_API int bscgpu_qlfc_front_batch_device(bscgpu_ctx* c, const void* dL, const int* sizes, int count, bscgpu_front_layout* out)
{
    if (!c) return LIBBSC_BAD_PARAMETER;
    const int arc = front_layout_args(sizes, count, out);
    if (arc < 0) return arc;
    int64_t total = 0;
    for (int b = 0; b < count; ++b) total += sizes[b];
    if (total > c->max_n || (total > 0 && !dL)) return LIBBSC_BAD_PARAMETER;
    if (hipSetDevice(c->device) != hipSuccess) return LIBBSC_GPU_ERROR;
    // the kernels read 16 bytes per lane: the pass goes through the context's own (aligned) L buffer, where the sorters leave it
    if (total > 0 && dL != c->dL && hipMemcpyAsync(c->dL, dL, (size_t)total, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
    std::vector<uint64_t> scratch(front_scratch_bytes(c->max_n) / 8 + 1);
    const int rc = qlfc_front_batch(c, c->dL, sizes, count, out, scratch.data());
    if (rc < 0) return rc;
    const uint32_t* first_run = reinterpret_cast<const uint32_t*>(scratch.data());
    for (int s = 0; s < out->nsub; ++s) qlfc_front_first_seen(first_run + 256 * (size_t)s, out->first_seen + 256 * (size_t)s, &out->nsym[s]);
    return LIBBSC_NO_ERROR;
}

static int64_t pstream_batch_device(bscgpu_ctx* c, const void* dL, const int* sizes, int count, bscgpu_front_layout* out,
                                    uint16_t* ps, int64_t cap, uint32_t* poff, int coder)
{
    if (!c || !poff || cap < 0 || (cap > 0 && !ps)) return LIBBSC_BAD_PARAMETER;
    const int frc = bscgpu_qlfc_front_batch_device(c, dL, sizes, count, out);
    if (frc < 0) return frc;
    poff[0] = 0;
    if (out->nsub == 0) return 0;
    u32 D = 0;
    const int rc = devcoder_pstream_batch(c, (u32)out->m, out->nsub, coder, &D);
    if (rc == LIBBSC_NOT_SUPPORTED) {
        char buf[96]; snprintf(buf, sizeof buf, "device coder declined the pass (reason mask %d)", c->dc_note.fail);
        c->err = buf;
    }
    if (rc < 0) return rc;
    if (hipMemcpyAsync(poff, devcoder_batch_poff_ptr(c), ((size_t)out->nsub + 1) * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
    if ((int64_t)D <= cap && D > 0 && hipMemcpyAsync(ps, devcoder_pstream_ptr(c, 0), (size_t)D * 2, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
    if (ctx_sync(c) != hipSuccess) return LIBBSC_GPU_ERROR;
    return (int64_t)D;
}
extern "C" BSCGPU_API int64_t bscgpu_static_pstream_batch_device(bscgpu_ctx* c, const void* dL, const int* sizes, int count, bscgpu_front_layout* out,
                                                                 uint16_t* ps, int64_t cap, uint32_t* poff)
{
    return pstream_batch_device(c, dL, sizes, count, out, ps, cap, poff, LIBBSC_CODER_QLFC_STATIC);
}
extern "C" BSCGPU_API int64_t bscgpu_fast_pstream_batch_device(bscgpu_ctx* c, const void* dL, const int* sizes, int count, bscgpu_front_layout* out,
                                                               uint16_t* ps, int64_t cap, uint32_t* poff)
{
    return pstream_batch_device(c, dL, sizes, count, out, ps, cap, poff, LIBBSC_CODER_QLFC_FAST);
}
extern "C" BSCGPU_API int64_t bscgpu_adaptive_pstream_batch_device(bscgpu_ctx* c, const void* dL, const int* sizes, int count, bscgpu_front_layout* out,
                                                                   uint16_t* ps, int64_t cap, uint32_t* poff, uint16_t* dbg)
{
    const int64_t D = pstream_batch_device(c, dL, sizes, count, out, ps, cap, poff, LIBBSC_CODER_QLFC_ADAPTIVE);
    if (D <= 0 || D > cap || !dbg) return D;
    for (int p = 0; p < 4; ++p)                                      // the device's planes are [4][D], the caller's [4][cap]
        if (hipMemcpyAsync(dbg + (size_t)p * (size_t)cap, devcoder_mix_dbg_ptr(c) + (size_t)p * (size_t)D, (size_t)D * 2, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            return LIBBSC_GPU_ERROR;
    if (ctx_sync(c) != hipSuccess) return LIBBSC_GPU_ERROR;
    return D;
}

extern "C" BSCGPU_API int64_t bscgpu_static_pstream_batch_packed_device(bscgpu_ctx* c, const void* dL, const int* sizes, int count, bscgpu_front_layout* out,
                                                                        uint8_t* packed, int64_t cap_bytes, uint32_t* poff, int64_t* pbase)
{
    if (!c || !poff || !pbase || cap_bytes < 0 || (cap_bytes > 0 && !packed)) return LIBBSC_BAD_PARAMETER;
    const int frc = bscgpu_qlfc_front_batch_device(c, dL, sizes, count, out);
    if (frc < 0) return frc;
    poff[0] = 0; pbase[0] = 0;
    if (out->nsub == 0) return 0;
    u32 D = 0;
    int pk = 0; int64_t bytes = 0;
    int rc = devcoder_pstream_batch(c, (u32)out->m, out->nsub, LIBBSC_CODER_QLFC_STATIC, &D, &pk, &bytes);
    if (rc == LIBBSC_NOT_SUPPORTED) {
        char buf[96]; snprintf(buf, sizeof buf, "device coder declined the pass (reason mask %d)", c->dc_note.fail);
        c->err = buf;
    }
    if (rc < 0) return rc;
    if (!pk) { c->err = "the packed stream of the pass was void (a wavefront's piece beyond the staging buffer)"; return LIBBSC_NOT_SUPPORTED; }
    std::vector<uint32_t> pb((size_t)out->nsub + 1);
    if (hipMemcpyAsync(poff, devcoder_batch_poff_ptr(c), ((size_t)out->nsub + 1) * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
    if (hipMemcpyAsync(pb.data(), devcoder_batch_pbase_ptr(c), ((size_t)out->nsub + 1) * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
    if (bytes <= cap_bytes && bytes > 0 && hipMemcpyAsync(packed, devcoder_pstream_ptr(c, 0), (size_t)bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
    if (ctx_sync(c) != hipSuccess) return LIBBSC_GPU_ERROR;
    for (int s = 0; s <= out->nsub; ++s) pbase[s] = (int64_t)pb[s];
    return (int64_t)D;
}

// ---- a single block in sub-block segments: the plan as a pure function (include/bscgpu.h) ------------------------------------------
extern "C" BSCGPU_API int bscgpu_block_segment_plan(const uint32_t* sub_runs, const uint32_t* sub_dec, int nsub, int64_t mcap, int64_t dcap, int* seg_of)
{
    return dc_block_segment_plan(sub_runs, sub_dec, nsub, mcap, dcap, seg_of);
}

// ---- a pass's model in segments (include/bscgpu.h) ---------------------------------------------------------------------------------
extern "C" BSCGPU_API int bscgpu_model_segment_plan(const uint32_t* sub_dec, const uint32_t* sub_und, const int* blk_sub, int count, int64_t dcap,
                                                    int64_t target, int* seg_of)
{
    if (count < 0 || dcap <= 0 || (count > 0 && (!sub_dec || !sub_und || !blk_sub || !seg_of))) return LIBBSC_BAD_PARAMETER;
    if (count > 0 && blk_sub[0] < 0) return LIBBSC_BAD_PARAMETER;
    for (int b = 0; b < count; ++b) if (blk_sub[b + 1] < blk_sub[b]) return LIBBSC_BAD_PARAMETER;
    return dc_segment_plan(sub_dec, sub_und, blk_sub, count, dcap, target, seg_of);
}

extern "C" BSCGPU_API int bscgpu_model_segment_facts_device(bscgpu_ctx* c, const void* dL, const int* sizes, int count, bscgpu_front_layout* out,
                                                            int coder, uint32_t* sub_dec, uint32_t* sub_und)
{
    if (!c || (count > 0 && (!sub_dec || !sub_und))) return LIBBSC_BAD_PARAMETER;
    if (coder != LIBBSC_CODER_QLFC_STATIC && coder != LIBBSC_CODER_QLFC_FAST) return LIBBSC_BAD_PARAMETER;
    const int frc = bscgpu_qlfc_front_batch_device(c, dL, sizes, count, out);
    if (frc < 0 || out->nsub == 0) return frc;
    return devcoder_segment_facts(c, (u32)out->m, out->nsub, coder, sub_dec, sub_und);
}

// ... for the adaptive coder (-e2): the third fact beside the static coder's two
extern "C" BSCGPU_API int bscgpu_adaptive_segment_facts_device(bscgpu_ctx* c, const void* dL, const int* sizes, int count, bscgpu_front_layout* out,
                                                               uint32_t* sub_dec, uint32_t* sub_und, uint32_t* sub_mix)
{
    if (!c || (count > 0 && (!sub_dec || !sub_und || !sub_mix))) return LIBBSC_BAD_PARAMETER;
    const int frc = bscgpu_qlfc_front_batch_device(c, dL, sizes, count, out);
    if (frc < 0 || out->nsub == 0) return frc;
    return devcoder_segment_facts(c, (u32)out->m, out->nsub, LIBBSC_CODER_QLFC_ADAPTIVE, sub_dec, sub_und, sub_mix);
}

// the stage in either form: pbase non-null is the packed one (out / cap in bytes); the callers have checked their own arguments
static int64_t pstream_batch_segments(bscgpu_ctx* c, const void* dL, const int* sizes, int count, bscgpu_front_layout* out, int coder, int64_t target,
                                      void* ps, int64_t cap, uint32_t* poff, int64_t* pbase, int* blk_state)
{
    const int frc = bscgpu_qlfc_front_batch_device(c, dL, sizes, count, out);
    if (frc < 0) return frc;
    poff[0] = 0;
    if (pbase) pbase[0] = 0;
    for (int b = 0; b < count; ++b) blk_state[b] = 0;
    if (out->nsub == 0) return 0;
    int64_t D = 0;
    const int rc = devcoder_pstream_segments(c, (u32)out->m, out->nsub, out->blk_sub, count, out->sub_run, coder, target, ps, cap, false, poff, blk_state, &D, nullptr, pbase);
    if (rc == LIBBSC_NOT_SUPPORTED) c->err = "device coder: an arena of the segmented model did not fit";
    if (rc < 0) return rc;
    return D;
}

extern "C" BSCGPU_API int64_t bscgpu_pstream_batch_segments_device(bscgpu_ctx* c, const void* dL, const int* sizes, int count, bscgpu_front_layout* out,
                                                                   int coder, int64_t target, uint16_t* ps, int64_t cap, uint32_t* poff, int* blk_state)
{
    if (!c || !poff || cap < 0 || (cap > 0 && !ps) || (count > 0 && !blk_state)) return LIBBSC_BAD_PARAMETER;
    if (coder != LIBBSC_CODER_QLFC_STATIC && coder != LIBBSC_CODER_QLFC_FAST) return LIBBSC_BAD_PARAMETER;
    return pstream_batch_segments(c, dL, sizes, count, out, coder, target, ps, cap, poff, nullptr, blk_state);
}

extern "C" BSCGPU_API int64_t bscgpu_adaptive_pstream_batch_segments_device(bscgpu_ctx* c, const void* dL, const int* sizes, int count, bscgpu_front_layout* out,
                                                                            int64_t target, uint16_t* ps, int64_t cap, uint32_t* poff, int* blk_state)
{
    if (!c || !poff || cap < 0 || (cap > 0 && !ps) || (count > 0 && !blk_state)) return LIBBSC_BAD_PARAMETER;
    return pstream_batch_segments(c, dL, sizes, count, out, LIBBSC_CODER_QLFC_ADAPTIVE, target, ps, cap, poff, nullptr, blk_state);
}

extern "C" BSCGPU_API int64_t bscgpu_pstream_batch_segments_packed_device(bscgpu_ctx* c, const void* dL, const int* sizes, int count, bscgpu_front_layout* out,
                                                                          int coder, int64_t target, uint8_t* packed, int64_t cap_bytes, uint32_t* poff,
                                                                          int64_t* pbase, int* blk_state)
{
    if (!c || !poff || !pbase || cap_bytes < 0 || (cap_bytes > 0 && !packed) || (count > 0 && !blk_state)) return LIBBSC_BAD_PARAMETER;
    if (coder != LIBBSC_CODER_QLFC_STATIC) return LIBBSC_BAD_PARAMETER;
    return pstream_batch_segments(c, dL, sizes, count, out, coder, target, packed, cap_bytes, poff, pbase, blk_state);
}

namespace {
// a pass's front-end layout (BatchPass): the small arrays here, sym / rank / start and the first-run table in a pinned buffer
struct PassLayout {
    bscgpu_front_layout lay;
    std::vector<int> sizes, blk_sub, sub_start, sub_size, nsym;
    std::vector<uint32_t> sub_run;
    std::vector<uint8_t> first_seen;
    const uint32_t* first_run = nullptr;
    bool used = false;
    const uint16_t* ps = nullptr;      // the device model's stream of the pass (BSCGPU_OPT_BATCH_MODEL), sub-block s at poff[s]; null: host model
    std::vector<uint32_t> poff;
    std::vector<int64_t> pbase;        // BSCGPU_OPT_BATCH_MODEL_PACKED: non-empty where ps (or the device's stream) is the packed 13-bit form, sub-block s at pbase[s]
    std::vector<int> blk_state;        // a pass in model segments (BSCGPU_OPT_BATCH_MODEL_SEGMENTS): != 0 where the block takes the host model; else empty
    // ... or, with BSCGPU_OPT_DEVICE_RC, the sub-blocks' coded bytes from the device's range coder: sub-block s's rc_res[s] bytes (or
    // LIBBSC_NOT_COMPRESSIBLE) at rc_bytes + rc_off[s], coded with an output budget of rc_room[s]
    const uint8_t* rc_bytes = nullptr;
    std::vector<uint32_t> rc_off;
    std::vector<int> rc_res, rc_room;
    void bind(const std::vector<int>& psz, uint8_t* pinned, size_t N)
    {
        const size_t cnt = psz.size();
        sizes = psz;
        blk_sub.assign(cnt + 1, 0); sub_start.assign(2 * cnt, 0); sub_size.assign(2 * cnt, 0); nsym.assign(2 * cnt, 0);
        sub_run.assign(2 * cnt + 1, 0); first_seen.resize(512 * cnt);
        lay = bscgpu_front_layout();
        lay.blk_sub = blk_sub.data(); lay.sub_start = sub_start.data(); lay.sub_size = sub_size.data(); lay.nsym = nsym.data();
        lay.sub_run = sub_run.data(); lay.first_seen = first_seen.data();
        lay.sym = pinned; lay.rank = pinned + N; lay.start = reinterpret_cast<uint32_t*>(pinned + 2 * N);
        first_run = reinterpret_cast<const uint32_t*>(pinned + 6 * N);
    }
};
}

int bschost::coder_threads() { return default_coder_threads(); }

// Smallest pass (bytes of L) that is given to the device model: below it the model's fixed cost (about a hundred launches, three
// syncs, the stream's copy) is more than the host spends on the pass's model.  Measured ("The static coder's model of a
// pass": tools/batch_bench.py --model-sweep): a call of one pass loses up to 8 MiB and wins from 16 MiB.
// BSC_BATCH_MODEL_MIN_PASS in the environment overrides it (read per call: the sweep and the tests run with 0).
// The fast coder's route (BSCGPU_OPT_BATCH_MODEL_FAST) has a minimum of its own from its own sweep ("The fast coder's
// model of a pass"): a call of one pass loses at every swept size, 64 KiB .. 16 MiB, so no swept size qualifies; the minimum is the
// next power of two above the sweep, below the 64 MiB passes of the several-pass calls that gain.  The environment variable
// overrides both.
constexpr int64_t BATCH_MODEL_MIN_PASS_DEFAULT = 16 << 20;
constexpr int64_t BATCH_MODEL_FAST_MIN_PASS_DEFAULT = 32 << 20;
static int64_t batch_model_min_pass(bool fast)
{
    const char* e = getenv("BSC_BATCH_MODEL_MIN_PASS");
    return e ? (int64_t)atoll(e) : fast ? BATCH_MODEL_FAST_MIN_PASS_DEFAULT : BATCH_MODEL_MIN_PASS_DEFAULT;
}

// A pass in model segments is coded in GROUPS of blocks, queued while its model still runs: first the blocks the device leaves out
// (their run arrays are down already), then each segment's blocks as its entries land.  One queue per pass slot; the pass's coder
// thread drains it, one group at a time, after its predecessor's pass is coded (PassOrder, which every pass's coding moves on).
struct PassGroups {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::vector<int>> groups;
    bool closed = false;
    void reset() { std::lock_guard<std::mutex> g(mu); groups.clear(); closed = false; }
    void push(std::vector<int>&& blk) { if (blk.empty()) return; { std::lock_guard<std::mutex> g(mu); groups.push_back(std::move(blk)); } cv.notify_all(); }
    void close() { { std::lock_guard<std::mutex> g(mu); closed = true; } cv.notify_all(); }
    bool pop(std::vector<int>& blk)
    {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return closed || !groups.empty(); });
        if (groups.empty()) return false;
        blk = std::move(groups.front()); groups.pop_front();
        return true;
    }
};
// what fills a segmented pass's queue: the segment driver's notes (DcSegNote), each block queued once
struct PassFeed {
    PassGroups* G; const std::vector<BatchBlock>* blocks; const int* blk_sub; const int* state; std::vector<char> queued;
    void take(int b0, int b1, bool planned)
    {
        std::vector<int> g;
        for (int i = b0; i < b1; ++i) {
            const BatchBlock& B = (*blocks)[i];
            // the first group: what the device's model leaves out, or never sees as a segment's member
            const bool member = B.cls == BATCH_SORTED && blk_sub[i + 1] > blk_sub[i];
            if (queued[i] || (planned && member && state[i] == 0)) continue;
            queued[i] = 1; g.push_back(i);
        }
        G->push(std::move(g));
    }
    static void planned(void* u) { PassFeed* f = static_cast<PassFeed*>(u); f->take(0, (int)f->blocks->size(), true); }
    static void settled(void* u, int b0, int b1) { static_cast<PassFeed*>(u)->take(b0, b1, false); }
};
struct PassOrder {
    std::mutex mu;
    std::condition_variable cv;
    int coded = 0;                 // passes of the call that are fully coded (they finish in order)
    void finish() { { std::lock_guard<std::mutex> g(mu); ++coded; } cv.notify_all(); }
    void wait_for(int passes) { std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return coded >= passes; }); }
};

// Decisions per model segment (BSCGPU_OPT_BATCH_MODEL_SEGMENTS): the device model's capacity (0).  That is the outcome of the sweep
// over the capacity / 8 .. the capacity (tools/batch_bench.py --segment-sweep): on W2 with host input no smaller value beats the
// capacity by more than the legs' own spread ("Model segments").  BSC_BATCH_MODEL_SEGMENT in the environment overrides it.
constexpr int64_t BATCH_MODEL_SEGMENT_DEFAULT = 0;
static int64_t batch_model_segment()
{
    const char* e = getenv("BSC_BATCH_MODEL_SEGMENT");
    return e ? (int64_t)atoll(e) : BATCH_MODEL_SEGMENT_DEFAULT;
}

// BSCGPU_OPT_DEVICE_RC for a model pass: every sub-block stream of the pass through ONE launch of the device's range coder
// (rangecoder.hip), eight streams per wavefront (DESIGN §3.8's table: the best shape for thousands of short streams), straight from
// the device's p stream.  Prefixes (header word, alphabet) come from bscgpu_rc_prefix per sub-block; the output regions lie in the
// sorter's first key buffer, dead until the next pass's sort (8 max_n bytes; the regions take n + 128 nsub at most); only the regions
// and res[] come down.  A sub-block is coded with the budget both framing rules give it when nothing in front of it was stored raw:
// its size, or n - 1 for a block of one sub-block.
static int device_rc_pass(bscgpu_ctx* c, PassLayout& PL, uint8_t* host_bytes, size_t host_cap, int coder)
{
    const bscgpu_front_layout& Y = PL.lay;
    const int nsub = Y.nsub;
    std::vector<uint32_t> prefix;
    std::vector<bscgpu_rc_stream> S((size_t)nsub);
    PL.rc_off.assign((size_t)nsub, 0); PL.rc_res.assign((size_t)nsub, 0); PL.rc_room.assign((size_t)nsub, 0);
    uint32_t off = 0;
    for (int b = 0; b < Y.count; ++b) {
        const int s0 = Y.blk_sub[b], nb = Y.blk_sub[b + 1] - s0;
        for (int s = s0; s < s0 + nb; ++s) {
            qlfc_front_first_seen(PL.first_run + 256 * (size_t)s, Y.first_seen + 256 * (size_t)s, &Y.nsym[s]);
            const size_t at = prefix.size();
            prefix.resize(at + BSCGPU_RC_PREFIX_MAX);
            const int np = bscgpu_rc_prefix(Y.first_seen + 256 * (size_t)s, Y.nsym[s], Y.sub_size[s], coder, prefix.data() + at, BSCGPU_RC_PREFIX_MAX);
            if (np < 0) return np;
            prefix.resize(at + (size_t)np);
            PL.rc_room[s] = nb == 1 ? Y.sub_size[s] - 1 : Y.sub_size[s];
            S[s].body = PL.pbase.empty() ? (int64_t)PL.poff[s] : PL.pbase[s]; S[s].count = PL.poff[s + 1] - PL.poff[s];
            S[s].prefix = (uint32_t)at; S[s].nprefix = (uint32_t)np;
            S[s].out_off = off; S[s].out_size = (uint32_t)PL.rc_room[s];
            PL.rc_off[s] = off;
            off += ((uint32_t)Y.sub_size[s] + 64u + 63u) & ~63u;
        }
    }
    if ((size_t)off > (size_t)8 * (size_t)c->max_n || (size_t)off > host_cap) return LIBBSC_NOT_SUPPORTED;
    uint8_t* dOut = reinterpret_cast<uint8_t*>(c->kA);
    const int rc = rc_encode_device(c, coder == LIBBSC_CODER_QLFC_FAST ? BSCGPU_RC_FAST16 : !PL.pbase.empty() ? BSCGPU_RC_STATIC13 : BSCGPU_RC_STATIC16, devcoder_pstream_ptr(c, 0), prefix.data(), (int)prefix.size(), S.data(), nsub, dOut, PL.rc_res.data(), 8);
    if (rc < 0) return rc;
    if (hipMemcpyAsync(host_bytes, dOut, (size_t)off, hipMemcpyDeviceToHost, c->stream) != hipSuccess || ctx_sync(c) != hipSuccess) return LIBBSC_GPU_ERROR;
    PL.rc_bytes = host_bytes;
    return LIBBSC_NO_ERROR;
}

// ---- the driver of a batched-compress call: what batch_pass_plan.h decides, done in named steps ------------------------------------
namespace {
// What every step of a call works on.  One implementation for both entry points: host input (`input`, LZP per block) or input in HBM
// (`dInput`; LZP, if any, on the device: dlzp).
struct BatchCall {
    bscgpu_ctx* c;
    const unsigned char* input; const unsigned char* dInput; const int* sizes; int count; unsigned char* output; int* results;
    int lzpHashSize, lzpMinLen, blockSorter, coder, features;
    int mode;
    bool dev, st;                                 // input in HBM; (make_mode: BWT or ST3..ST8) the pass is one sort transform, no aux indexes
    std::vector<int> pass_of;
    std::vector<int64_t> in_off;
    BatchRoute route;
    size_t frontN;
    int threads;
    std::vector<char> single;                     // blocks that are not coded with a pass: batch_leftovers
    std::vector<uint32_t> res, adler;             // what the sort of a pass leaves, until finish_blocks (one pass sorts at a time)
    std::vector<int> stidx;
    bool dlzp = false;                            // LZP of a pass's members is one run of the device's stage over the raw pass (BatchPass::stage_lzp), not lzp_compress
                                                  // per block: input in HBM with LZP, or host input with BSCGPU_OPT_BATCH_DEVICE_LZP and parameters the stage takes
    bool lzp_declined = false;                    // ... the option is on, the stage does not take the parameters: the passes keep host LZP

    const unsigned char* in_of(int b) const { return input + in_off[b]; }
    const unsigned char* din_of(int b) const { return dInput + in_off[b]; }
    unsigned char* out_of(int b) const { return output + in_off[b] + (int64_t)LIBBSC_HEADER_SIZE * b; }
    bool lzp() const { return block_mode_has_lzp(mode); }
    int alone(int b) const                        // a block by the single-block path on the call's context
    {
        return dev ? bscgpu_compress_device_lzp(c, din_of(b), out_of(b), sizes[b], lzpHashSize, lzpMinLen, blockSorter, coder, features)
                   : compress_one_on_ctx(c, in_of(b), out_of(b), sizes[b], lzpHashSize, lzpMinLen, blockSorter, coder, features);
    }
};

class PassHandOff;

// A pass of a call, in one of the call's two slots (p & 1; PassHandOff says why the slot is free): its blocks [b, e) of the input, where
// they lie in the pass, its front-end layout and the queue its coding is fed from when the model runs in segments.
struct BatchPass {
    BatchCall* K = nullptr;
    int p = 0, b = 0, e = 0;
    std::vector<BatchBlock> blocks;
    BatchGeometry G;                              // (G.at[i]: where block b + i's L lies in hb)
    u8* hb = nullptr;
    PassLayout PL;
    PassGroups groups;
    bool finished = false, grouped = false;

    void prepare(BatchCall* call, int pass, int b0, int e0);
    void prep_block(int i);
    int  stage();
    int  stage_lzp();
    int  sort();
    int  l_down();
    int  front();
    BatchModelStep model_step();
    int  model_whole();
    int  land_whole(u32 D, int pk, int64_t pbytes);
    int  model_segments(PassHandOff& hand);
    void finish_blocks();
    // what the coding of the pass is made of: one block; the whole pass; the pass in groups (model segments)
    PassSource source_of(int i) const;
    void code_block(int i);
    void code_pass(PassOrder& order);
    void code_groups(PassOrder& order);
};

// The threads of a call.  One coder thread per pass codes pass p while pass p + 1 sorts; the thread of a pass in model segments starts
// early, beside the pass's model, and becomes its coder thread when the pass is handed over; PassOrder makes the passes finish in order.
// The buffer-lifetime rule: what pass p writes — its BatchPass slot and the context's batch_host, front_host and model_host of the same
// index p & 1 — is free because the coder thread of pass p - 2 was joined (in take() of pass p - 1) before pass p - 1's coding started.
class PassHandOff {
public:
    PassOrder order;
    // a pass in model segments: its groups are coded as they are queued, from now on
    void start_early(BatchPass& P)
    {
        P.grouped = true;
        try { early_thread = std::thread([&P, this] { P.code_groups(order); }); }
        catch (const std::system_error&) {}           // no thread to be had: the groups are coded in take(), after the model
    }
    // the pass is sorted and its blocks are finished: the previous pass's coding ends here, this pass's runs beside the next pass's sort
    void take(BatchPass& P)
    {
        if (coder_thread.joinable()) coder_thread.join();
        if (P.grouped) {                              // its coding is under way (or waits here, where no thread was to be had)
            if (early_thread.joinable()) coder_thread = std::move(early_thread);
            else P.code_groups(order);
            return;
        }
        try { coder_thread = std::thread([&P, this] { P.code_pass(order); }); }
        catch (const std::system_error&) { P.code_pass(order); }                   // no thread to be had: code the pass here
    }
    // the end of the call (a pass that ended in an error: its thread codes what it was given and ends)
    void finish(BatchPass* slots)
    {
        slots[0].groups.close(); slots[1].groups.close();
        if (coder_thread.joinable()) coder_thread.join();
        if (early_thread.joinable()) early_thread.join();
    }
private:
    std::thread coder_thread;                     // codes the previous pass while this one sorts
    std::thread early_thread;                     // ... this pass's, when it started before the pass's model had finished (model segments)
};

void ctx_count(bscgpu_ctx* c, const BatchCounters& d)
{
    c->cnt_front_passes += d.front_passes; c->cnt_l_passes += d.l_passes;
    c->cnt_model_passes += d.model_passes; c->cnt_model_declined += d.model_declined;
    c->cnt_model_fast_passes += d.fast_passes; c->cnt_model_fast_declined += d.fast_declined;
    c->cnt_model_adaptive_passes += d.adaptive_passes; c->cnt_model_adaptive_declined += d.adaptive_declined;
    c->cnt_packed_passes += d.packed_passes; c->cnt_packed_void += d.packed_void; c->cnt_device_rc += d.device_rc;
}

// 1. prepare: the pass takes its slot; LZP of every member (libbsc.cpp:263-281) and its class
void BatchPass::prepare(BatchCall* call, int pass, int b0, int e0)
{
    K = call; p = pass; b = b0; e = e0;
    blocks.assign((size_t)(e - b), BatchBlock());
    finished = grouped = false;
    PL.used = false;
    groups.reset();
    hb = K->c->batch_host[p & 1];
    if (K->lzp_declined) ++K->c->cnt_lzp_declined;
    // in parallel; without LZP on the host there is nothing to spread over threads
    if (K->lzp() && !K->dlzp) run_bounded(e - b, K->threads, [this](int i) { prep_block(i); });
    else for (int i = 0; i < e - b; ++i) prep_block(i);
}

void BatchPass::prep_block(int i)
{
    BatchBlock& B = blocks[i];
    const int q = b + i, n = K->sizes[q];
    B.b = q; B.mode = K->mode; B.lz = n;
    B.cls = batch_block_class(n, n, K->st, K->dev, K->pass_of[q] >= 0);            // (before LZP: n stands for what it leaves)
    if (B.cls == BATCH_STORED) K->results[q] = bsc_store(K->in_of(q), K->out_of(q), n, K->features);
    if (B.cls != BATCH_SORTED || !K->lzp() || K->dlzp) return;      // (dlzp: the member stays raw, stage_lzp settles lz, mode and class)
    B.lzbuf = (unsigned char*)bigbuf_get((size_t)n);
    const int r = B.lzbuf ? lzp_compress(K->in_of(q), B.lzbuf, n, K->lzpHashSize, K->lzpMinLen, K->features) : LIBBSC_NOT_ENOUGH_MEMORY;
    if (r < LIBBSC_NO_ERROR) { B.mode = block_mode_without_lzp(B.mode); bigbuf_put(B.lzbuf); B.lzbuf = nullptr; }
    else B.lz = r;
    B.cls = batch_block_class(n, B.lz, K->st, K->dev, true);
    if (B.cls == BATCH_SINGLE) { bigbuf_put(B.lzbuf); B.lzbuf = nullptr; }
}

// 2. stage: where every block lies in the pass; host input goes into hb and up to the device
int BatchPass::stage()
{
    if (K->dlzp) return stage_lzp();
    const int cnt = e - b;
    std::vector<BatchClass> cls((size_t)cnt);
    std::vector<int> lz((size_t)cnt);
    for (int i = 0; i < cnt; ++i) { cls[i] = blocks[i].cls; lz[i] = blocks[i].lz; }
    batch_pass_geometry(cls.data(), K->sizes + b, lz.data(), cnt, K->st, K->dev, &G);
    if (K->dev) return LIBBSC_NO_ERROR;                                          // the pass is the caller's own range of HBM
    for (int i = 0; i < cnt; ++i) {
        BatchBlock& B = blocks[i];
        if (B.cls == BATCH_SORTED) memcpy(hb + G.at[i], B.lzbuf ? B.lzbuf : K->in_of(B.b), (size_t)B.lz);
        if (B.lzbuf) { bigbuf_put(B.lzbuf); B.lzbuf = nullptr; }
    }
    if (G.pos > 0 && hipMemcpyAsync(K->c->dL, hb, (size_t)G.pos, hipMemcpyHostToDevice, K->c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
    return LIBBSC_NO_ERROR;
}

// 2'. stage, LZP on the device: the raw pass — the caller's own range of HBM, or the same range of host input uploaded to dT — goes
// through one run of the LZP stage (lzp.hip: lzp_batch_device), whose frame kernel lays the sorter's input out in dL as the host
// route would: the sorted blocks' streams back to back, a block the stage finds not compressible with its raw bytes and without LZP
// in its mode (libbsc.cpp:266-269), a block that rides along with its raw bytes.  Input in HBM: the checksums of the original blocks
// come from one segmented launch over the raw pass, before the sort (which is then called without its checksum output).
int BatchPass::stage_lzp()
{
    bscgpu_ctx* c = K->c;
    const int cnt = e - b;
    const int* sz = K->sizes + b;
    const int64_t range = K->in_off[e] - K->in_off[b];
    const u8* raw = K->dev ? K->din_of(b) : c->dT;
    if (!K->dev && range > 0) {
        memcpy(hb, K->in_of(b), (size_t)range);
        if (hipMemcpyAsync(c->dT, hb, (size_t)range, hipMemcpyHostToDevice, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
    }
    if (K->dev) {
        const int trc = batch_tab_ensure(c);
        if (trc < 0) return trc;
        std::vector<u32> off((size_t)cnt + 1, 0u);
        for (int i = 0; i < cnt; ++i) off[(size_t)i + 1] = off[(size_t)i] + (u32)sz[i];
        u32* dadler = c->batch_tab + 18 * BATCH_MAX_BLOCKS + 1;                     // (batch_pass_setup's place for them; the sort comes later)
        if (hipMemcpyAsync(c->batch_tab, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
        launch_adler_batch(c, raw, c->batch_tab, (u32)cnt, dadler);
        if (hipMemcpyAsync(K->adler.data(), dadler, (size_t)cnt * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
    }
    std::vector<int> lzres((size_t)cnt);
    int sorted = 0;
    const LzpBatchPlace place = [&](const int* res, uint32_t* dst, unsigned char* as_it_is) {
        std::vector<BatchClass> cls((size_t)cnt);
        std::vector<int> lz((size_t)cnt);
        for (int i = 0; i < cnt; ++i) {
            BatchBlock& B = blocks[i];
            if (B.cls == BATCH_SORTED) {
                if (res[i] < LIBBSC_NO_ERROR) B.mode = block_mode_without_lzp(B.mode); else B.lz = res[i];
                B.cls = batch_block_class(sz[i], B.lz, K->st, K->dev, true);
            }
            cls[i] = B.cls; lz[i] = B.lz;
        }
        batch_pass_geometry(cls.data(), sz, lz.data(), cnt, K->st, false, &G, true);
        for (int i = 0; i < cnt; ++i) {
            if (cls[i] != BATCH_SORTED && cls[i] != BATCH_RIDES) continue;
            dst[i] = (uint32_t)G.at[i];
            as_it_is[i] = cls[i] == BATCH_RIDES || res[i] < LIBBSC_NO_ERROR;
            sorted += cls[i] == BATCH_SORTED;
        }
    };
    const int rc = lzp_batch_device(c, raw, c->dL, sz, cnt, K->lzpHashSize, K->lzpMinLen, K->features, lzres.data(), false, &place);
    if (rc < 0) return rc;
    ++c->cnt_batch_lzp_passes; c->cnt_batch_lzp_blocks += sorted;
    return LIBBSC_NO_ERROR;
}

// 3. sort: one suffix sort or one sort transform for the pass
int BatchPass::sort()
{
    bscgpu_ctx* c = K->c;
    const bool in_place = K->dev && !K->dlzp;                                   // (dlzp: the pass is what stage_lzp left in dL, checksums taken)
    const u8* src = in_place ? K->din_of(b) : c->dL;
    u32* adler = in_place ? K->adler.data() : nullptr;
    return K->st ? st_batch_device(c, src, c->dL, G.psz.data(), e - b, K->blockSorter, G.prate.data(), K->stidx.data(), adler)
                 : bwt_batch_device(c, src, c->dL, G.psz.data(), e - b, G.prate.data(), K->res.data(), adler);
}

// 5c. L down: the pass's L comes back in one copy
int BatchPass::l_down()
{
    bscgpu_ctx* c = K->c;
    if (hipMemcpyAsync(hb, c->dL, (size_t)G.pos, hipMemcpyDeviceToHost, c->stream) != hipSuccess || ctx_sync(c) != hipSuccess) return LIBBSC_GPU_ERROR;
    ++c->cnt_l_passes;
    return LIBBSC_NO_ERROR;
}

// 4. front: the pass's run arrays come down instead of its L
int BatchPass::front()
{
    bscgpu_ctx* c = K->c;
    // (the front end covers the whole range of the pass: with HBM input that includes members the layout is never read
    // for — a block left to the single path rides along untransformed; correct, a little wasted work)
    PL.bind(G.psz, c->front_host[p & 1], K->frontN);
    const int rc = qlfc_front_batch(c, c->dL, PL.sizes.data(), e - b, &PL.lay, c->front_host[p & 1] + 6 * K->frontN);
    if (rc < 0) return rc;
    PL.used = true; ++c->cnt_front_passes;
    PL.ps = nullptr; PL.rc_bytes = nullptr; PL.blk_state.clear(); PL.pbase.clear();
    return rc;
}

// ... and which model step follows it; the two pinned stream buffers are allocated by the first pass that qualifies
BatchModelStep BatchPass::model_step()
{
    BatchModelStep step = batch_model_step(K->route, PL.lay.nsub, G.pos, true);
    if (step != BATCH_MODEL_NONE && ctx_ensure_model_host(K->c) != LIBBSC_NO_ERROR) step = batch_model_step(K->route, PL.lay.nsub, G.pos, false);
    return step;
}

// 5a. model whole: the model behind the front end, on the same stream, before the next pass's sort; the run arrays came down all the
// same: they serve a declined pass, a sub-block stored raw and the <= 28-byte blocks that rode along
int BatchPass::model_whole()
{
    bscgpu_ctx* c = K->c;
    u32 D = 0;
    int pk = 0; int64_t pbytes = 0;          // packed: what the device left is the 13-bit form, pbytes of it; void: 16-bit entries as ever
    const int mrc = devcoder_pstream_batch(c, (u32)PL.lay.m, PL.lay.nsub, K->coder, &D, K->route.packed ? &pk : nullptr, &pbytes);
    const BatchVerdict v = batch_whole_verdict(mrc, D, pk, pbytes, c->model_host_entries);
    if (v == BATCH_PASS_ERROR) return mrc;
    if (v == BATCH_PASS_KEPT) {
        const int rc = land_whole(D, pk, pbytes);
        if (rc < 0) return rc;
    }
    ctx_count(c, batch_model_counters(K->route, BATCH_MODEL_WHOLE, v, pk));
    return LIBBSC_NO_ERROR;
}

// the kept stream of a whole pass comes down — or stays in HBM, where one launch of the device's range coder codes it
int BatchPass::land_whole(u32 D, int pk, int64_t pbytes)
{
    bscgpu_ctx* c = K->c;
    PL.poff.resize((size_t)PL.lay.nsub + 1);
    u16* hps = c->model_host[p & 1];
    const bool drc = K->route.device_rc;
    const size_t down = pk ? (size_t)pbytes : (size_t)D * 2;
    std::vector<uint32_t> pb(pk ? PL.poff.size() : 0);
    if (hipMemcpyAsync(PL.poff.data(), devcoder_batch_poff_ptr(c), PL.poff.size() * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        (pk && hipMemcpyAsync(pb.data(), devcoder_batch_pbase_ptr(c), pb.size() * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        (!drc && down > 0 && hipMemcpyAsync(hps, devcoder_pstream_ptr(c, 0), down, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        ctx_sync(c) != hipSuccess) return LIBBSC_GPU_ERROR;
    if (pk) PL.pbase.assign(pb.begin(), pb.end());
    if (drc) return device_rc_pass(c, PL, reinterpret_cast<uint8_t*>(hps), c->model_host_entries * 2, K->coder);
    PL.ps = hps;
    return LIBBSC_NO_ERROR;
}

// 5b. model segments: the same route segment by segment: the streams of the kept blocks land back to back, a block the device leaves
// out (or whose segment no longer fits the landing buffer) is coded from its run arrays.  Coding starts with the plan: the pass's
// thread takes groups of blocks as they settle (PassGroups)
int BatchPass::model_segments(PassHandOff& hand)
{
    bscgpu_ctx* c = K->c;
    const bool packed = K->route.packed;
    const int cnt = e - b;
    PL.poff.resize((size_t)PL.lay.nsub + 1);
    PL.blk_state.assign((size_t)cnt, 0);
    PL.ps = c->model_host[p & 1];
    if (packed) PL.pbase.assign((size_t)PL.lay.nsub + 1, 0);
    finish_blocks();
    PassFeed feed{&groups, &blocks, PL.lay.blk_sub, PL.blk_state.data(), std::vector<char>((size_t)cnt, 0)};
    DcSegNote note{PassFeed::planned, PassFeed::settled, &feed};
    hand.start_early(*this);
    int64_t D = 0;
    // (packed: the landing buffer in bytes, less the few a packed entry's 4-byte read may reach past a stream)
    const int mrc = devcoder_pstream_segments(c, (u32)PL.lay.m, PL.lay.nsub, PL.lay.blk_sub, cnt, PL.lay.sub_run, K->coder, K->route.segment_target,
                                              c->model_host[p & 1], packed ? (int64_t)c->model_host_entries * 2 - 8 : (int64_t)c->model_host_entries,
                                              true, PL.poff.data(), PL.blk_state.data(), &D, &note, packed ? PL.pbase.data() : nullptr);
    const BatchVerdict v = batch_segments_verdict(mrc, PL.lay.blk_sub, PL.blk_state.data(), cnt);
    if (v == BATCH_PASS_ERROR) { groups.close(); return mrc; }
    // (an arena did not fit: what is not queued yet takes the host model)
    if (mrc < 0) for (int i = 0; i < cnt; ++i) if (!feed.queued[i]) PL.blk_state[i] = BSCGPU_DC_FAIL_CAP;
    ctx_count(c, batch_model_counters(K->route, BATCH_MODEL_SEGMENTS, v, 0));
    feed.take(0, cnt, false);               // whatever is left
    groups.close();
    return LIBBSC_NO_ERROR;
}

// 6. finish blocks: the sort's results into the blocks, before the first of them is coded
void BatchPass::finish_blocks()
{
    if (finished) return;
    finished = true;
    for (int i = 0; i < e - b; ++i) {
        BatchBlock& B = blocks[i];
        if (B.cls == BATCH_SINGLE) K->single[B.b] = 1;
        if (K->dev) B.adler = K->adler[i];
        if (B.cls != BATCH_SORTED) continue;
        if (K->st) { B.index = K->stidx[i]; B.num_indexes = 0; continue; }
        const uint32_t* I = K->res.data() + 16 * (size_t)i;
        B.index = (int)I[0];
        B.num_indexes = (B.lz - 1) / aux_rate(B.lz);
        for (int t = 0; t < B.num_indexes; ++t) B.indexes[t] = (int)I[t + 1] - 1;
    }
}

// (the per-block test "this block keeps the host model" is settled here)
PassSource BatchPass::source_of(int i) const
{
    const bool host_block = !PL.blk_state.empty() && PL.blk_state[i] != 0, packed = !PL.pbase.empty();
    PassSource S = {};
    S.kind = batch_block_source(PL.used, PL.ps != nullptr, PL.rc_bytes != nullptr, host_block, K->coder == LIBBSC_CODER_QLFC_FAST, packed);
    S.L = hb + G.at[i];
    S.lay = &PL.lay; S.li = i;
    S.ps = PL.ps; S.poff = PL.poff.data(); S.pbase = PL.pbase.data();
    S.rc_bytes = PL.rc_bytes; S.rc_off = PL.rc_off.data(); S.rc_res = PL.rc_res.data(); S.rc_room = PL.rc_room.data();
    S.packed = packed;
    return S;
}

void BatchPass::code_block(int i)
{
    const BatchBlock& B = blocks[i];
    if (B.cls != BATCH_RIDES && B.cls != BATCH_SORTED) return;
    const int n = K->sizes[B.b];
    const bscgpu_front_layout& Y = PL.lay;
    if (PL.used)
        for (int s = Y.blk_sub[i]; s < Y.blk_sub[i + 1]; ++s)
            qlfc_front_first_seen(PL.first_run + 256 * (size_t)s, Y.first_seen + 256 * (size_t)s, &Y.nsym[s]);
    if (B.cls == BATCH_RIDES) {             // <= 28 bytes that rode along (L = T): in the pass's L, or — its bytes are its runs — in its layout
        unsigned char tmp[LIBBSC_HEADER_SIZE + 1];
        RunView V[8];
        if (PL.used) { front_views(&Y, i, V); expand_runs(V[0], 0, tmp); }
        K->results[B.b] = bsc_store(PL.used ? tmp : hb + G.at[i], K->out_of(B.b), n, K->features);
        return;
    }
    const PassSource S = source_of(i);
    K->results[B.b] = code_sorted_block(K->c, K->dev ? nullptr : K->in_of(B.b), K->dev ? K->din_of(B.b) : nullptr, K->out_of(B.b), n, B, K->coder, K->features, &S);
}

void BatchPass::code_pass(PassOrder& order)
{
    run_bounded((int)blocks.size(), K->threads, [this](int i) { code_block(i); });
    order.finish();
}

// one coding group at a time per call: the previous pass's coding first, then this pass's groups as they are queued
void BatchPass::code_groups(PassOrder& order)
{
    order.wait_for(p);
    std::vector<int> g;
    while (groups.pop(g)) run_bounded((int)g.size(), K->threads, [&](int k) { code_block(g[k]); });
    order.finish();
}

// the call's route: the context's options and the coder, with the environment's values read per call
BatchRoute call_route(bscgpu_ctx* c, int npass, int coder)
{
    const BatchOptions o = {c->batch_front, c->batch_model, c->batch_model_fast, c->batch_model_segments, c->batch_model_packed, c->device_rc, c->batch_model_adaptive,
                            c->batch_adaptive_segments};
    // the front end needs the two pinned run buffers; without them today's route
    const bool front_host = batch_wants_front(npass, o) && ctx_ensure_front_host(c) == LIBBSC_NO_ERROR;
    return batch_route(npass, o, coder, front_host, batch_model_min_pass(false), batch_model_min_pass(true), batch_model_segment());
}

// the plan of the call, its offsets, buffers and route -> the number of passes, or a negative code
int batch_call_begin(BatchCall& K)
{
    bscgpu_ctx* c = K.c;
    K.pass_of.resize((size_t)K.count);
    const int npass = plan_for(K.sizes, K.count, K.blockSorter, c->max_n, K.pass_of.data());
    if (npass < 0) return npass;
    K.in_off.assign((size_t)K.count + 1, 0);
    for (int b = 0; b < K.count; ++b) K.in_off[b + 1] = K.in_off[b] + K.sizes[b];
    if (npass > 0)
        for (int k = 0; k < 2; ++k)
            if (!c->batch_host[k] && hipHostMalloc((void**)&c->batch_host[k], (size_t)c->max_n + 64, hipHostMallocDefault) != hipSuccess) {
                c->batch_host[k] = nullptr;
                return ctx_fail(c, LIBBSC_GPU_NOT_ENOUGH_MEMORY, "batched compression: pinned pass buffers", hipSuccess);
            }
    K.route = call_route(c, npass, K.coder);
    K.frontN = ((size_t)c->max_n + 4096 + 4095) / 4096 * 4096;
    K.threads = default_coder_threads();
    K.single.assign((size_t)K.count, 0);
    for (int b = 0; b < K.count; ++b) K.single[b] = K.pass_of[b] < 0;
    K.res.resize((size_t)BATCH_MAX_BLOCKS * 16); K.adler.resize((size_t)BATCH_MAX_BLOCKS); K.stidx.resize((size_t)BATCH_MAX_BLOCKS);
    return npass;
}

// The blocks of their own, beside the last pass's coding: through a pipe on this context (the GPU stage of one overlaps the host
// coding of the ones before it); the few it does not take (larger than the context, a too short sorter input) first, one by one
// (both use the context's pinned slots: never at the same time)
void batch_leftovers(BatchCall& K)
{
    // (input in HBM with LZP: the pipe's HBM entry has no LZP form, every block left over goes through bscgpu_compress_device_lzp)
    auto kind = [&](int b) {
        const BatchLeftover k = batch_leftover(K.single[b] != 0, K.pass_of[b] >= 0, K.sizes[b], K.c->max_n, K.dev);
        return k == BATCH_LEFT_PIPE && K.dev && K.lzp() ? BATCH_LEFT_ONE_BY_ONE : k;
    };
    auto one_by_one = [&](BatchLeftover k) { for (int b = 0; b < K.count; ++b) if (kind(b) == k) K.results[b] = K.alone(b); };
    one_by_one(BATCH_LEFT_ONE_BY_ONE);
    bool any = false;
    for (int b = 0; b < K.count; ++b) any = any || kind(b) == BATCH_LEFT_PIPE;
    if (!any) return;
    bscgpu_pipe* pipe = nullptr;
    constexpr int PIPE_DEPTH = 4;
    if (bscgpu_pipe_create(K.c, PIPE_DEPTH, &pipe) < 0) { one_by_one(BATCH_LEFT_PIPE); return; }        // no pipe: one by one
    std::deque<std::pair<int, int>> inflight;         // (block, ticket)
    for (int b = 0; b < K.count; ++b) {
        if (kind(b) != BATCH_LEFT_PIPE) continue;
        if ((int)inflight.size() >= PIPE_DEPTH) { K.results[inflight.front().first] = bscgpu_pipe_wait(pipe, inflight.front().second); inflight.pop_front(); }
        const int t = K.dev ? bscgpu_pipe_submit(pipe, K.din_of(b), K.out_of(b), K.sizes[b], K.blockSorter, K.coder, K.features)
                            : bscgpu_pipe_submit_host(pipe, K.in_of(b), K.out_of(b), K.sizes[b], K.lzpHashSize, K.lzpMinLen, K.blockSorter, K.coder, K.features);
        if (t < 0) K.results[b] = t; else inflight.push_back({b, t});
    }
    for (auto& ft : inflight) K.results[ft.first] = bscgpu_pipe_wait(pipe, ft.second);
    bscgpu_pipe_destroy(pipe);
}
}  // namespace

static int compress_batch_impl(bscgpu_ctx* c, const unsigned char* input, const unsigned char* dInput, const int* sizes, int count,
                               unsigned char* output, int* results, int lzpHashSize, int lzpMinLen, int blockSorter, int coder, int features)
{
    BatchCall K = {c, input, dInput, sizes, count, output, results, lzpHashSize, lzpMinLen, blockSorter, coder, features, 0,
                   dInput != nullptr, blockSorter != LIBBSC_BLOCKSORTER_BWT, {}, {}, {}, 0, 0, {}, {}, {}, {}};
    const int mrc = make_mode(blockSorter, coder, lzpHashSize, lzpMinLen, &K.mode);
    if (mrc != LIBBSC_NO_ERROR) { for (int b = 0; b < count; ++b) results[b] = mrc; return LIBBSC_NO_ERROR; }
    const bool takes = device_lzp_takes(lzpHashSize);
    if (K.dev && K.lzp() && !takes) return LIBBSC_NOT_SUPPORTED;                 // as bscgpu_compress_device_lzp: the stage holds a chunk's table in LDS
    K.dlzp = K.lzp() && takes && (K.dev || c->batch_device_lzp != 0);
    K.lzp_declined = !K.dev && K.lzp() && !takes && c->batch_device_lzp != 0;
    if (hipSetDevice(c->device) != hipSuccess) return LIBBSC_GPU_ERROR;
    const int npass = batch_call_begin(K);
    if (npass < 0) return npass;
    BatchPass slots[2];
    PassHandOff hand;
    int rc = LIBBSC_NO_ERROR;
    // (a negative rc ends the passes: the threads that were started code what they were given, blocks already coded keep their results)
    for (int b = 0, p = 0; b < count && rc >= 0;) {
        if (K.pass_of[b] < 0) { ++b; continue; }
        const int e = batch_pass_end(K.pass_of.data(), sizes, count, b);
        BatchPass& P = slots[p & 1];
        P.prepare(&K, p, b, e);
        rc = P.stage();
        const bool sorts = rc >= 0 && P.G.pos > 0;                                 // (host input of stored blocks only: nothing to sort)
        if (sorts) rc = P.sort();
        if (sorts && rc >= 0) rc = K.route.front ? P.front() : P.l_down();
        if (sorts && rc >= 0 && K.route.front)
            switch (P.model_step()) {
            case BATCH_MODEL_WHOLE:    rc = P.model_whole(); break;
            case BATCH_MODEL_SEGMENTS: rc = P.model_segments(hand); break;
            case BATCH_MODEL_NONE:     break;
            }
        if (rc < 0) break;
        P.finish_blocks();
        hand.take(P);
        b = e; ++p;
    }
    if (rc >= 0) batch_leftovers(K);
    hand.finish(slots);
    return rc;
}


static int batch_args(bscgpu_ctx* c, const void* in, const int* sizes, int count, unsigned char* output, int* results)
{
    if (!c || count < 0 || (count > 0 && (!sizes || !output || !results))) return LIBBSC_BAD_PARAMETER;
    int64_t total = 0;
    for (int b = 0; b < count; ++b) { if (sizes[b] < 0) return LIBBSC_BAD_PARAMETER; total += sizes[b]; }
    if (total > 0 && !in) return LIBBSC_BAD_PARAMETER;
    return LIBBSC_NO_ERROR;
}

extern "C" BSCGPU_API int bscgpu_compress_batch(bscgpu_ctx* c, const unsigned char* input, const int* sizes, int count, unsigned char* output,
                                                int* results, int lzpHashSize, int lzpMinLen, int blockSorter, int coder, int features)
{
    const int rc = batch_args(c, input, sizes, count, output, results);
    if (rc < 0 || count == 0) return rc;
    return compress_batch_impl(c, input, nullptr, sizes, count, output, results, lzpHashSize, lzpMinLen, blockSorter, coder, features);
}

// Input in HBM: the passes are sorted straight from the caller's buffer, every block's Adler-32 comes from one segmented launch per
// pass (st.hip: adler_batch_kernel); only L and, for a block that ends up stored, its own bytes cross PCIe.
extern "C" BSCGPU_API int bscgpu_compress_batch_device(bscgpu_ctx* c, const void* dInput, const int* sizes, int count, unsigned char* output,
                                                       int* results, int blockSorter, int coder, int features)
{
    const int rc = batch_args(c, dInput, sizes, count, output, results);
    if (rc < 0 || count == 0) return rc;
    static const unsigned char empty = 0;       // (a batch of empty blocks may come with no buffer at all)
    return compress_batch_impl(c, nullptr, dInput ? (const unsigned char*)dInput : &empty, sizes, count, output, results, 0, 0,
                               blockSorter, coder, features);
}

extern "C" BSCGPU_API int bscgpu_compress_batch_device_lzp(bscgpu_ctx* c, const void* dInput, const int* sizes, int count, unsigned char* output,
                                                           int* results, int lzpHashSize, int lzpMinLen, int blockSorter, int coder, int features)
{
    if (lzpHashSize == 0 && lzpMinLen == 0) return bscgpu_compress_batch_device(c, dInput, sizes, count, output, results, blockSorter, coder, features);
    const int rc = batch_args(c, dInput, sizes, count, output, results);
    if (rc < 0 || count == 0) return rc;
    static const unsigned char empty = 0;
    return compress_batch_impl(c, nullptr, dInput ? (const unsigned char*)dInput : &empty, sizes, count, output, results, lzpHashSize, lzpMinLen,
                               blockSorter, coder, features);
}
