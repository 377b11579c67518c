"""CPU checks of the native side of several resident LPs' rounds in one call (csrc/gcnn_lprounds.hpp, csrc/k_lprounds.hpp): its
symbols are in the header, the binding and the built library at ABI 13; its launch names are its own; every twin kernel
cross-compiles for gfx950 without scratch and with no more LDS than the solo kernel whose body it runs; the layout query lays
mixed members out as the contract says; and every bad argument and limit is returned before anything could be enqueued."""
import ctypes as C
import os
import re

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
LPROUNDS = os.path.join(CSRC, "gcnn_lprounds.hpp")
SYMBOLS = ("gcnn_lp_rounds_layout_for", "gcnn_lp_rounds")
# twin -> the solo kernel whose body it runs (as the resource remarks name it)
TWINS = {"k_lprs_round_stats": "k_lpr_stats6LpArgs7LprArgs", "k_lprs_round_emit": "k_lpr_emit6LpArgs10LpEmitMore",
         "k_lprs_append_stats": "k_lpa_stats", "k_lprs_append_scan": "k_lpa_scan", "k_lprs_append_move": "k_lpa_move",
         "k_lprs_append_order": "k_lpa_order", "k_lprs_rank_scores": "k_rank_scoresPKfiPi", "k_lprs_sel_pairs": "k_sel_pairs7SelArgs",
         "k_lprs_sel_filter": "k_sel_filter7SelArgs"}
SCORES, RANK, SELECT = 0, 1, 2


def test_symbols_in_header_binding_and_library_abi_13():
    from gcnn_cut_selector_amd import _lib
    header = buildsupport.declared_everywhere(SYMBOLS)
    assert _lib.ABI_VERSION == 13 and _lib.lib().gcnn_abi_version() == 13          # the ABI is additive: the number does not move
    for struct in ("gcnn_lp_rounds_member", "gcnn_lp_rounds_layout"):
        assert struct in header
    assert "#define GCNN_LP_ROUNDS_MAX GCNN_GROUP_MAX" in header and _lib.LP_ROUNDS_MAX == _lib.GROUP_MAX == 8
    P, Z = C.sizeof(C.c_void_p), C.sizeof(C.c_size_t)
    assert C.sizeof(_lib.LpRoundsMember) == C.sizeof(_lib.LpDims) + 16 + C.sizeof(_lib.LpAppendDims) + 9 * P
    assert C.sizeof(_lib.LpRoundsLayout) == 8 + (8 + 8 * 8) * Z
    fields = re.search(r"typedef struct gcnn_lp_rounds_layout \{(.*?)\} gcnn_lp_rounds_layout;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert tuple(re.findall(r"(\w+)(?:\[\w+\])?\s*[;,]", fields)) == tuple(n for n, _ in _lib.LpRoundsLayout._fields_)


def _own_names():
    src = re.sub(r"//[^\n]*", "", open(LPROUNDS).read())
    return set(re.findall(r'"(k_[a-z_0-9]+)"', src))         # (whole literals: the table's names, not the include)


def test_launch_names_are_its_own():
    names = _own_names()
    assert names == set(TWINS)
    assert len(launchnames.launch_names()) == 28 and not names & launchnames.launch_names()
    for other in sorted(os.listdir(CSRC)):
        if other.startswith("gcnn_") and other.endswith(".hpp") and other != "gcnn_lprounds.hpp":
            text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, other)).read())
            assert not names & (launchnames.launch_names(os.path.join(CSRC, other)) | set(re.findall(r'"(k_[^"]*)"', text))), other
    assert not launchnames.launch_names(LPROUNDS)             # its launches go out through the group's launcher, under the twins' names
    buildsupport.included_once_after("gcnn_lprounds.hpp", "gcnn_select.hpp", "gcnn_lpstate.hpp", "gcnn_group.hpp", "gcnn_lpres.hpp",
                                     "gcnn_lpappend.hpp")
    kernels = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "k_lprounds.hpp")).read())
    assert set(re.findall(r"__global__[^\n;{]*?\bvoid (\w+)\(", kernels)) == names
    # a twin carries the name it is launched under, and no name of another family's filters
    assert not [n for n in names if any(p in n for p in ("k_group_", "k_lpr_", "k_lpa_", "k_lp_", "k_sel_", "k_rank_"))]


def test_twins_compile_without_scratch_and_within_the_solo_lds():
    build = buildsupport.device_build()
    rows = build.rows
    twins = {k: v for k, v in rows.items() if "k_lprs_" in k}
    assert len(twins) == len(TWINS) and {re.search(r"k_lprs_[a-z_]+?(?=PK9GroupHead)", k).group(0) for k in twins} == set(TWINS), sorted(twins)
    for name, v in twins.items():
        twin = re.search(r"k_lprs_[a-z_]+?(?=PK9GroupHead)", name).group(0)
        solo = [r for k, r in rows.items() if TWINS[twin] in k and "k_lprs_" not in k]
        assert len(solo) == 1, (twin, [k for k in rows if TWINS[twin] in k])
        assert v["scratch"] == 0 and v["lds"] <= solo[0]["lds"] and v["occ"] >= solo[0]["occ"], (name, v, solo[0])
        assert build.wavefront_size(name) == 64
    assert len([k for k in rows if "k_group_" in k]) == 35        # the forward pass's family is unchanged


def _dims(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_rows=100, n_cols=50, n_cuts=7, row_nnz=400, cut_nnz=33, has_incumbent=1, n_model_vars=50, n_state_rows=130,
             n_state_edges=520, reserved=0, infinity=1e20, sum_epsilon=1e-6, obj_norm=2.0)
    f.update(over)
    return _lib.LpDims(**f)


def _block(**over):
    from gcnn_cut_selector_amd import _lib
    f = dict(n_rows=10, row_nnz=45, n_state_rows=14, n_state_edges=60, n_lhs_rows=6, n_lhs_edges=25, res_lhs_rows=60, res_lhs_edges=250)
    f.update(over)
    return _lib.LpAppendDims(**f)


def _member(dims=None, present=3, nf=-1, nfe=0, block=None, base=1 << 30, keep=None):
    """A member whose pointers are never dereferenced: spaced apart from every other member's by `base`."""
    from gcnn_cut_selector_amd import _lib
    m = _lib.LpRoundsMember()
    m.dims = dims if dims is not None else _dims()
    m.present, m.n_forced, m.n_forced_entries = present, nf, nfe
    step = 1 << 24
    at = [base + step * i for i in range(48)]
    res = _lib.LpResident(*at[:9], _lib.Graph(*at[9:15], 0, 0))
    sets = [_lib.LpRowsSet(*at[16:26]), _lib.LpRowsSet(*at[26:36])]
    if block is not None:
        m.has_append, m.block = 1, block
        m.row_ptr, m.row_col, m.row_val, m.row_lhs, m.row_rhs = at[36:41]
        m.src, m.dst = C.pointer(sets[0]), C.pointer(sets[1])
        res.cons_feats, res.row_place, res.row_scale = sets[1].cons_feats, sets[1].row_place, sets[1].row_scale
    m.resident = C.pointer(res)
    m.params = at[41]
    if keep is not None:
        keep.extend([res] + sets)
    return m


def _array(members):
    from gcnn_cut_selector_amd import _lib
    return (_lib.LpRoundsMember * len(members))(*members)


def test_layout_of_mixed_members():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    keep = []
    specs = [dict(nf=2, nfe=9), dict(nf=0, nfe=0, block=_block()), dict(nf=1, nfe=3, dims=_dims(n_cuts=0, cut_nnz=0)),
             dict(nf=0, nfe=0, block=_block(n_rows=300, row_nnz=900, n_state_rows=300, n_state_edges=900, n_lhs_rows=0, n_lhs_edges=0)),
             dict(nf=3, nfe=4, dims=_dims(n_rows=257, n_state_rows=257, row_nnz=600, n_state_edges=600), present=15)]
    members = [_member(base=(i + 1) << 32, keep=keep, **s) for i, s in enumerate(specs)]
    n = len(members)
    L = _lib.LpRoundsLayout()
    assert lib.gcnn_lp_rounds_layout_for(n, _array(members), SELECT, C.byref(L)) == 0
    assert L.n == n and L.mode == SELECT
    solo_in, solo_out, solo_arena = [], [], []
    for m in members:
        if m.has_append:
            A = _lib.LpAppendLayout()
            assert lib.gcnn_lp_append_layout_for(C.byref(m.dims), C.byref(m.block), m.present, m.n_forced, m.n_forced_entries, C.byref(A)) == 0
            solo_in.append(A.in_bytes); solo_out.append(A.out_bytes); solo_arena.append(A.arena_bytes)
        else:
            R = _lib.LpRoundLayout()
            assert lib.gcnn_lp_round_layout_for(C.byref(m.dims), m.present, m.n_forced, m.n_forced_entries, C.byref(R)) == 0
            solo_in.append(R.in_bytes); solo_out.append(R.out_bytes); solo_arena.append(R.arena_bytes)
    # uploads: contiguous from 0, in member order, each the solo upload within 255 bytes of alignment
    at = 0
    for i in range(n):
        assert L.in_off[i] == at and L.in_off[i] % 256 == 0 and solo_in[i] <= L.in_size[i] <= solo_in[i] + 255
        at += L.in_size[i]
    assert L.in_bytes == at
    # downloads: contiguous from out_base, each the solo download
    at = 0
    for i in range(n):
        assert L.out_off[i] == at and L.out_size[i] == solo_out[i] and L.out_off[i] % 16 == 0
        at += L.out_size[i]
    assert L.out_bytes == at and L.out_base % 256 == 0
    # every region inside the arena, none overlapping another
    regions = [(0, L.in_bytes), (L.out_base, L.out_base + L.out_bytes), (L.table_off, L.table_off + L.table_bytes)]
    regions += [(L.arena_off[i], L.arena_off[i] + solo_arena[i]) for i in range(n)]
    if L.counts_bytes:
        regions.append((L.counts_base, L.counts_base + L.counts_bytes))
    regions.sort()
    assert all(a[1] <= b[0] for a, b in zip(regions, regions[1:])) and regions[-1][1] <= L.arena_bytes, regions
    assert L.in_bytes <= L.arena_off[0] and max(L.arena_off[i] + solo_arena[i] for i in range(n)) <= L.counts_base <= L.out_base < L.table_off
    for i, m in enumerate(members):
        assert L.arena_off[i] % 256 == 0 and L.member_round_off[i] % 256 == 0
        if m.has_append:
            assert L.arena_off[i] < L.member_round_off[i] < L.scratch_off[i] < L.arena_off[i] + solo_arena[i]
            assert L.counts_base <= L.counts_off[i] < L.counts_base + L.counts_bytes and L.counts_off[i] % 16 == 0
        else:
            assert L.member_round_off[i] == L.arena_off[i] and L.scratch_off[i] == 0 and L.counts_off[i] == 0
    counts = sorted(L.counts_off[i] for i, m in enumerate(members) if m.has_append)
    assert counts[0] == L.counts_base and L.counts_bytes >= 2 * (8 * 50 + 4)          # the appends' count tables, side by side: one fill
    assert L.table_off % 256 == 0 and L.table_bytes > 0
    # without an append there is nothing to fill
    assert lib.gcnn_lp_rounds_layout_for(1, _array(members[:1]), SELECT, C.byref(L)) == 0 and L.counts_bytes == 0
    # n, mode, the members' own limits
    many = [_member(base=(i + 1) << 32, keep=keep) for i in range(9)]
    assert lib.gcnn_lp_rounds_layout_for(0, _array(many), SCORES, C.byref(L)) == -1
    assert lib.gcnn_lp_rounds_layout_for(9, _array(many), SCORES, C.byref(L)) == -1
    assert lib.gcnn_lp_rounds_layout_for(8, _array(many), SCORES, C.byref(L)) == 0
    assert lib.gcnn_lp_rounds_layout_for(2, _array(many), 3, C.byref(L)) == -1 and lib.gcnn_lp_rounds_layout_for(2, _array(many), -1, C.byref(L)) == -1
    assert lib.gcnn_lp_rounds_layout_for(2, None, SCORES, C.byref(L)) == -1 and lib.gcnn_lp_rounds_layout_for(2, _array(many), SCORES, None) == -1
    assert lib.gcnn_lp_rounds_layout_for(2, _array(many), SELECT, C.byref(L)) == -1             # a selection needs every member's n_forced
    assert lib.gcnn_lp_rounds_layout_for(2, _array(members), SCORES, C.byref(L)) == -1          # and the other modes take none
    wide = _dims(n_cuts=4097, cut_nnz=5000)
    assert lib.gcnn_lp_rounds_layout_for(2, _array([many[0], _member(dims=wide, base=9 << 32, keep=keep)]), SCORES, C.byref(L)) == 0
    assert lib.gcnn_lp_rounds_layout_for(2, _array([many[0], _member(dims=wide, base=9 << 32, keep=keep)]), RANK, C.byref(L)) == -4
    assert lib.gcnn_lp_rounds_layout_for(2, _array([members[0], _member(dims=wide, nf=0, base=9 << 32, keep=keep)]), SELECT, C.byref(L)) == -4
    assert lib.gcnn_lp_rounds_layout_for(1, _array([_member(block=_block(n_rows=0), keep=keep)]), SCORES, C.byref(L)) == -1


def test_refusals_before_anything_is_enqueued():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    keep = []
    P = 1 << 20
    L = _lib.LpRoundsLayout()

    def call(members, mode=SCORES, n=None, hin=P, hout=P, arena=P << 8, bytes_=1 << 60, staging=P, p=(0.1, 0.5)):
        return lib.gcnn_lp_rounds(len(members) if n is None else n, _array(members), mode, hin, hout, arena, bytes_, staging, *p, None)

    pair = [_member(base=(i + 1) << 32, keep=keep) for i in range(2)]
    assert lib.gcnn_lp_rounds_layout_for(2, _array(pair), SCORES, C.byref(L)) == 0
    assert call(pair, n=0) == -1 and call([_member(base=(i + 1) << 32, keep=keep) for i in range(9)]) == -1
    assert call(pair, hin=0) == -1 and call(pair, hout=0) == -1 and call(pair, arena=0) == -1 and call(pair, staging=0) == -1
    assert call(pair, arena=(P << 8) + 128) == -1 and call(pair, bytes_=L.arena_bytes - 1) == -1 and call(pair, staging=P + 8) == -1
    sel = [_member(nf=0, base=(i + 1) << 32, keep=keep) for i in range(2)]
    assert call(sel, SELECT, p=(float("nan"), 0.5)) == -1 and call(sel, SELECT, p=(0.1, float("inf"))) == -1
    # a member's own pointers
    for spoil in ("params", "resident"):
        bad = _member(base=2 << 32, keep=keep)
        setattr(bad, spoil, None)
        assert call([pair[0], bad]) == -1, spoil
    hole = _member(base=2 << 32, keep=keep)
    hole.resident.contents.row_place = None
    assert call([pair[0], hole]) == -1
    app = _member(block=_block(), base=2 << 32, keep=keep)
    app.src = None
    assert call([pair[0], app]) == -1
    app = _member(block=_block(), base=2 << 32, keep=keep)
    app.row_ptr = None
    assert call([pair[0], app]) == -1
    # the limits of an ordering mode
    wide = _dims(n_cuts=4097, cut_nnz=5000)
    assert call([pair[0], _member(dims=wide, base=2 << 32, keep=keep)], RANK) == -4
    assert call([sel[0], _member(dims=wide, nf=0, base=2 << 32, keep=keep)], SELECT) == -4
    assert call([pair[0], _member(dims=_dims(n_cols=(1 << 24) + 1), base=2 << 32, keep=keep)]) == -4
    # one member's writable memory over another member's memory: the same session twice, a shared optional column buffer, an
    # append's destination over another member's resident rows, its raw rows over another member's parameters
    assert call([pair[0], _member(base=1 << 32, keep=keep)]) == -1
    shared = _member(base=2 << 32, keep=keep)
    shared.resident.contents.col_ub = pair[0].resident.contents.col_ub
    assert call([pair[0], shared]) == -1
    over = _member(block=_block(), base=2 << 32, keep=keep)
    over.dst.contents.v_oth = pair[0].resident.contents.row_scale
    assert call([pair[0], over]) == -1
    over = _member(block=_block(), base=2 << 32, keep=keep)
    over.row_val = pair[0].params
    assert call([pair[0], over]) == -1
