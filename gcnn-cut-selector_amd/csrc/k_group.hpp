// k_group.hpp -- grouped launches: one launch runs the same stage of up to GCNN_GROUP_MAX independent models' steps
// (gcnn_group_train_step, gcnn_group_forward; host side in gcnn_group.hpp).
//
// A member's step is recorded, not launched: the solo launchers run unchanged with a recorder installed (GCNN_LAUNCH), so every
// member keeps its own dispatch choices (edge slots, long-segment blocks, block-per-segment, split or four/eight-wave row
// programs) and its own grid.  Stage s of the group then goes out as one launch per distinct kernel among the members' s-th
// launches.  Its blocks are the members' solo grids back to back; a block finds its member in the launch's table (a prefix of
// block counts, at most 8 entries) and runs the solo body with that member's arguments and its solo (block, blocks) pair.  Every
// value that depends on the block partition -- the d w_edge partial rows, the weight-gradient slabs, the head partials, the
// reduction order -- is therefore the solo launch's: the bits are the solo step's.
//
// Table of one launch (device memory, uploaded with the whole step's tables in one copy): GroupHead, then n argument records of
// `stride` bytes each (the solo kernel's argument, or a GPair of its two arguments).

#include <tuple>

static_assert(GCNN_GROUP_MAX == 8, "include/gcnn_hip.h");
#define GCNN_GROUP_MAX_STAGES 16   // launches of one member's step (training: 15)

struct GroupHead { int n, stride; int blk0[GCNN_GROUP_MAX + 1]; int pad[5]; };
static_assert(sizeof(GroupHead) == 64, "argument records start 64-B aligned");
template <class A, class B> struct GPair { A a; B b; };
template <class A, class B, class D> struct GTriple { A a; B b; D c; };

// the member this block serves, its block index and block count within the member's share of the launch.  The table is read
// through the constant address space: the block-uniform loads then go to scalar registers as kernel arguments do (through a
// plain global pointer they take vector registers, and the row programs spill)
#define GROUP_CONST __attribute__((address_space(4)))
template <class P>
__device__ __forceinline__ const P& group_member(const GroupHead* t_, int& bid, int& nblk) {
    const GROUP_CONST GroupHead* t = (const GROUP_CONST GroupHead*)t_;
    const int x = blockIdx.x, n = t->n;
    int m = 0;
    for (int i = 1; i < n; ++i) m += x >= t->blk0[i];
    const int b0 = t->blk0[m];
    bid = x - b0;
    nblk = t->blk0[m + 1] - b0;
    return *(const P*)((const GROUP_CONST P*)((const GROUP_CONST char*)t + sizeof(GroupHead) + (size_t)m * t->stride));
}

// Each group kernel has its solo kernel's launch bounds and attributes, and runs the same body.
template <int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) __attribute__((amdgpu_waves_per_eu(NWAVES / 2, NWAVES / 2))) void k_group_embed_fwd(const GroupHead* __restrict__ t) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int b, nb;
    const EmbGroupArgs& m = group_member<EmbGroupArgs>(t, b, nb);
    embed_fwd_body<NWAVES>(m, smem, b);
}
__global__ __launch_bounds__(256) void k_group_embed_fwd_split(const GroupHead* __restrict__ t) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int b, nb;
    const EmbGroupArgs& m = group_member<EmbGroupArgs>(t, b, nb);
    embed_fwd_split_body(m, smem, b);
}
template <int SLOTS, bool COUNT, bool LONG>
__global__ __launch_bounds__(256) void k_group_edge_fwd(const GroupHead* __restrict__ t) {
    int b, nb;
    const GPair<EdgeArgs, int>& p = group_member<GPair<EdgeArgs, int>>(t, b, nb);
    edge_fwd_body<SLOTS, COUNT, LONG>(p.a, p.b, b, nb);
}
template <bool COUNT>
__global__ __launch_bounds__(256) void k_group_edge_fwd_block(const GroupHead* __restrict__ t) {
    int b, nb;
    const EdgeArgs& a = group_member<EdgeArgs>(t, b, nb);
    edge_fwd_block_body<COUNT>(a, b, nb);
}
template <int NWAVES, int TAIL>
__global__ __launch_bounds__(NWAVES * 64) void k_group_conv_fwd(const GroupHead* __restrict__ t) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int b, nb;
    const ConvFArgs& a = group_member<ConvFArgs>(t, b, nb);
    convf_program<TAIL, NWAVES * 64, false>(a, smem, b, nb);
}
template <int TAIL>
__global__ __launch_bounds__(256) void k_group_conv_fwd_split(const GroupHead* __restrict__ t) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int b, nb;
    const ConvFArgs& a = group_member<ConvFArgs>(t, b, nb);
    convf_split<TAIL, false>(a, smem, b, nb);
}
template <int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void k_group_conv_turn(const GroupHead* __restrict__ t) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int b, nb;
    const GPair<ConvFArgs, ConvBArgs>& p = group_member<GPair<ConvFArgs, ConvBArgs>>(t, b, nb);
    convturn_program<NWAVES * 64>(p.a, p.b, smem, b, nb);
}
__global__ __launch_bounds__(256) void k_group_conv_turn_split(const GroupHead* __restrict__ t) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int b, nb;
    const GPair<ConvFArgs, ConvBArgs>& p = group_member<GPair<ConvFArgs, ConvBArgs>>(t, b, nb);
    convturn_split(p.a, p.b, smem, b, nb);
}
template <int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void k_group_conv_bwd(const GroupHead* __restrict__ t) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int b, nb;
    const ConvBGroupArgs& m = group_member<ConvBGroupArgs>(t, b, nb);
    conv_bwd_body<NWAVES>(m, smem, b);
}
template <int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void k_group_tail_bwd(const GroupHead* __restrict__ t) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int b, nb;
    const TailGroupArgs& m = group_member<TailGroupArgs>(t, b, nb);
    tail_bwd_body<NWAVES>(m, smem, b);
}
template <int SLOTS, bool LONG>
__global__ __launch_bounds__(256) void k_group_edge_bwd_send(const GroupHead* __restrict__ t) {
    int b, nb;
    const GPair<EdgeArgs, int>& p = group_member<GPair<EdgeArgs, int>>(t, b, nb);
    edge_bwd_send_body<SLOTS, LONG>(p.a, p.b, b, nb);
}
__global__ __launch_bounds__(64 * WG_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_group_wgrad(const GroupHead* __restrict__ t) {
    extern __shared__ __attribute__((aligned(16))) float wg_red[];
    int b, nb;
    const GPair<WgArgs, DwRedArgs>& p = group_member<GPair<WgArgs, DwRedArgs>>(t, b, nb);
    wgrad_body(p.a, p.b, wg_red, b);
}
__global__ __launch_bounds__(256) void k_group_reduce(const GroupHead* __restrict__ t) {
    int b, nb;
    const GPair<RdArgs, FoldArgs>& p = group_member<GPair<RdArgs, FoldArgs>>(t, b, nb);
    reduce_body(p.a, p.b, b);
}

// ---- host: the recorder the solo launchers write into while a group step collects its members' launches -------------------
static constexpr size_t group_max(size_t a, size_t b) { return a > b ? a : b; }
#define GROUP_REC_BYTES                                                                                                        \
    group_max(group_max(group_max(sizeof(EmbGroupArgs), sizeof(GPair<EdgeArgs, int>)), group_max(sizeof(ConvFArgs), sizeof(GPair<ConvFArgs, ConvBArgs>))), \
              group_max(group_max(sizeof(ConvBGroupArgs), sizeof(TailGroupArgs)), group_max(sizeof(GPair<WgArgs, DwRedArgs>), sizeof(GPair<RdArgs, FoldArgs>))))
struct GroupRecord {
    const void* kern;   // the solo kernel: what the launch would have run
    int grid, block, bytes;
    size_t smem;
    alignas(16) unsigned char args[GROUP_REC_BYTES];
};
struct GroupRecorder { GroupRecord* rec; int n, cap; bool bad; };
// installed on this thread while a member's step is recorded (nullptr: the launchers launch)
static thread_local GroupRecorder* g_group_rec = nullptr;

// false: not a kernel a group step records (the single-state inference launches never are)
template <class V>
static bool group_put(GroupRecord& q, const V& v) {
    if constexpr (sizeof(V) > sizeof(q.args)) return false;
    else { memcpy(q.args, &v, sizeof(V)); q.bytes = (int)sizeof(V); return true; }
}
template <class... P, class... A>
static void group_record(GroupRecorder* r, void (*k)(P...), dim3 grid, dim3 block, size_t smem, A&&... args) {
    if (r->n >= r->cap) { r->bad = true; return; }
    GroupRecord& q = r->rec[r->n++];
    q.kern = (const void*)k; q.grid = (int)grid.x; q.block = (int)block.x; q.smem = smem;
    bool ok;
    if constexpr (sizeof...(P) == 1) { using P1 = typename std::tuple_element<0, std::tuple<P...>>::type; ok = group_put(q, P1(args...)); }
    else if constexpr (sizeof...(P) == 2) {
        using P1 = typename std::tuple_element<0, std::tuple<P...>>::type;
        using P2 = typename std::tuple_element<1, std::tuple<P...>>::type;
        const std::tuple<A&...> t(args...);
        ok = group_put(q, GPair<P1, P2>{P1(std::get<0>(t)), P2(std::get<1>(t))});
    } else if constexpr (sizeof...(P) == 3) {
        using P1 = typename std::tuple_element<0, std::tuple<P...>>::type;
        using P2 = typename std::tuple_element<1, std::tuple<P...>>::type;
        using P3 = typename std::tuple_element<2, std::tuple<P...>>::type;
        const std::tuple<A&...> t(args...);
        ok = group_put(q, GTriple<P1, P2, P3>{P1(std::get<0>(t)), P2(std::get<1>(t)), P3(std::get<2>(t))});
    } else ok = false;
    if (!ok) r->bad = true;
}
// HIP work on a member's path that a group step cannot record (a memset, a launch outside GCNN_LAUNCH): while recording, it
// marks the recording unusable (the group call then refuses with GCNN_E_UNSUPPORTED) instead of running ahead of the group
static bool group_unrecorded() {
    if (!g_group_rec) return false;
    g_group_rec->bad = true;
    return true;
}
static hipError_t group_memset(void* p, size_t bytes, hipStream_t st) {
    return group_unrecorded() ? hipSuccess : hipMemsetAsync(p, 0, bytes, st);
}
// the launchers of the training step and the forward pass launch through this: recorded while a group step collects its members
#define GCNN_LAUNCH(K, GRID, BLOCK, SMEM, ST, ...)                                                                     \
    do {                                                                                                                \
        if (g_group_rec) group_record(g_group_rec, K, GRID, BLOCK, SMEM, __VA_ARGS__);                                  \
        else hipLaunchKernelGGL(K, GRID, BLOCK, SMEM, ST, __VA_ARGS__);                                                 \
    } while (0)
