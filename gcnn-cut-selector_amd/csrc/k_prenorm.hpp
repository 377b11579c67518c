// k_prenorm.hpp -- the group twins of the kernels a PreNorm fitting call launches beyond a forward pass (gcnn_group_prenorm_merge;
// host side in gcnn_prenorm.hpp).  They work as the twins of k_group.hpp do: a block finds its member in the launch's table and
// runs the solo body with that member's arguments and its solo (block, blocks) pair.  Named k_pgroup_*: the k_group_* family is
// the training step's and the forward pass's.

// the two-layer form of the receiver-side update that keeps A (gcnn_forward with save_for_backward = 2)
template <int NWAVES, int TAIL>
__global__ __launch_bounds__(NWAVES * 64) void k_pgroup_conv_fwd(const GroupHead* __restrict__ t) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int b, nb;
    const ConvFArgs& a = group_member<ConvFArgs>(t, b, nb);
    convf_program<TAIL, NWAVES * 64, true>(a, smem, b, nb);
}
template <int TAIL>
__global__ __launch_bounds__(256) void k_pgroup_conv_fwd_split(const GroupHead* __restrict__ t) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int b, nb;
    const ConvFArgs& a = group_member<ConvFArgs>(t, b, nb);
    convf_split<TAIL, true>(a, smem, b, nb);
}
__global__ __launch_bounds__(256) void k_pgroup_expand_ptr(const GroupHead* __restrict__ t) {
    int b, nb;
    const ExpandArgs& a = group_member<ExpandArgs>(t, b, nb);
    expand_ptr_body(a, b, nb);
}
__global__ __launch_bounds__(256) void k_pgroup_stats(const GroupHead* __restrict__ t) {
    __shared__ double red[256];
    int b, nb;
    const StatArgs& a = group_member<StatArgs>(t, b, nb);
    stats_body(a, red, b, nb);
}
__global__ __launch_bounds__(64) void k_pgroup_stats_fold(const GroupHead* __restrict__ t) {
    int b, nb;
    const StatFoldArgs& a = group_member<StatFoldArgs>(t, b, nb);
    stats_fold_body(a);
}
static_assert(sizeof(StatArgs) <= GROUP_REC_BYTES && sizeof(StatFoldArgs) <= GROUP_REC_BYTES && sizeof(ExpandArgs) <= GROUP_REC_BYTES,
              "a recorded argument fits a GroupRecord");
