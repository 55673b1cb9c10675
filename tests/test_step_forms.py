"""CPU tests: which training-step kernel a call of emg_train_backward_ex would launch — the decision of emg_score.hip's
decide_step_form, asked through the dry run emg_train_backward_form (same checks, same decision, no launch, no pointer followed:
the pointers here are made-up addresses).  The expected forms are written out from the dispatch rules as they stood before the
decision was gathered in one function; the GPU tests (test_config_widths, test_cache_policy_forms, test_focuse, test_graph_step,
test_api) run the kernels themselves."""
import ctypes as C
import os

import pytest

from emgraph_amd import _lib as L

EINVAL, ENOSUP = -1, -3
PASS_BACKWARD, PASS_FUSED = 1, 2
CACHE_POLICY, LINKED, RIDE, ALONE = 1, 2, 4, 8
MODELS = [L.TRANSE_L1, L.TRANSE_L2, L.DISTMULT, L.COMPLEX, L.HOLE]
OPTS = {"sgd": L.OPT_SGD, "momentum": L.OPT_MOMENTUM, "adagrad": L.OPT_ADAGRAD, "adam": L.OPT_ADAM, "adam_lazy": L.OPT_ADAM_LAZY}


def _addr(i, off=0):
    return 0x100000 * (i + 1) + off


def make_args(model=L.DISTMULT, cols=32, B=4096, eta=5, fused=True, opt=None, lp=0, window=False, lr_hist=False, link=L.LINK_LINEAR,
              edge_w=False, misaligned=False, n_ent=1000, bw_scores=False):
    """a valid call: `cols` columns per row (per half for complex models); opt = None: no in-place updates"""
    a = L.BackwardArgs()
    k = 2 * cols if model in (L.COMPLEX, L.HOLE) else cols
    a.model, a.k_int, a.scale, a.eta = model, k, 1.0, eta
    a.ent, a.n_ent, a.ld_ent = _addr(0, 4 if misaligned else 0), n_ent, k
    a.rel, a.n_rel, a.ld_rel = _addr(1), 50, k
    a.pos, a.B, a.codes = _addr(2), B, _addr(3)
    a.contrib_ent, a.contrib_rel, a.ldc = _addr(4), _addr(5), k
    a.margin, a.step = 1.0, 3
    if fused:
        a.fused_loss, a.loss_accum, a.link = L.LOSS_NLL, _addr(6), link
        if edge_w:
            a.edge_w, a.sw = _addr(7), 0.5
    else:
        a.fused_loss, a.g_pos, a.g_neg = -1, _addr(8), _addr(9)
        if bw_scores:
            a.bw_scores_pos, a.bw_scores_neg = _addr(10), _addr(11)
    for i, v in enumerate([0.01, 0.9, 0.9, 0.999, 1e-7, 0.01, 0.0, 0.0]):
        a.hyper[i] = v
    if opt is not None:
        a.single_ent, a.opt, a.tag_ent = _addr(12), OPTS[opt], _addr(13)
        a.ent_state0, a.ent_state1 = (0 if opt == "sgd" else _addr(14)), (_addr(15) if opt in ("adam", "adam_lazy") else 0)
        if lp:
            a.hyper[6], a.hyper[7], a.lp_accum = 0.01, float(lp), _addr(16)
        a.inplace_window = 1 if window else 0
        if lr_hist:
            a.lr_hist = _addr(17)
    return a


def form(a, riders=0):
    """(rc, error text, [W, NV, LPG, in-place form, flags, blocks]) of the dry run; pass and model are checked here"""
    lib = L.load()
    out = (C.c_int32 * 8)()
    rc = lib.emg_train_backward_form(C.byref(a), riders, out)
    if rc != 0:
        return rc, lib.emg_last_error().decode(), None
    assert out[0] == (PASS_FUSED if a.fused_loss >= 0 else PASS_BACKWARD) and out[1] == a.model
    return 0, "", list(out[2:8])


def expect(a, W, NV, LPG, ip, flags=0, blocks=1, riders=0):
    rc, err, f = form(a, riders)
    assert rc == 0, err
    assert f == [W, NV, LPG, ip, flags, blocks], f


@pytest.fixture(autouse=True)
def _switches_unset(monkeypatch):
    monkeypatch.delenv("EMG_WIDE_GROUPS", raising=False)
    monkeypatch.delenv("EMG_CACHE_POLICY", raising=False)


# chunks of 16 bytes per row (per half for complex models) -> (chunks per lane, lanes per group): narrow rows share a wave at
# B > 2048, a wave per group at B <= 2048
VEC_LADDER_SHARED = {16: (1, 16), 17: (1, 32), 32: (1, 32), 33: (1, 64), 64: (1, 64), 65: (2, 64), 128: (2, 64)}
VEC_LADDER_WAVE = {16: (1, 64), 17: (1, 64), 32: (1, 64), 33: (1, 64), 64: (1, 64), 65: (2, 64), 128: (2, 64)}
# columns of a scalar row -> chunks (floats) per lane; always a wave per group
SCALAR_LADDER = {64: 1, 65: 2, 128: 2, 129: 4, 256: 4, 257: 8, 512: 8}


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("fused", [True, False])
def test_width_ladder_of_16_byte_rows(model, fused):
    for chunks, (nv, lpg) in VEC_LADDER_SHARED.items():
        expect(make_args(model, 4 * chunks, B=2049, fused=fused), 4, nv, lpg, 0)
    for chunks, (nv, lpg) in VEC_LADDER_WAVE.items():
        expect(make_args(model, 4 * chunks, B=2048, fused=fused), 4, nv, lpg, 0)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("fused", [True, False])
def test_width_ladder_of_scalar_rows(model, fused):
    for cols, nv in SCALAR_LADDER.items():
        for B in (2048, 2049):
            expect(make_args(model, cols, B=B, fused=fused, misaligned=True), 1, nv, 64, 0)   # (a table that is not 16-byte aligned)
    expect(make_args(model, 63, fused=fused), 1, 1, 64, 0)                                    # (no whole chunks)
    a = make_args(model, 64, fused=fused)
    a.ldc += 1                                                                                # (a stride that breaks the alignment)
    expect(a, 1, 1, 64, 0)


@pytest.mark.parametrize("env,B,lpg", [(None, 2048, 64), (None, 2049, 16), ("0", 2048, 16), ("0", 2049, 16), ("1", 2048, 64),
                                       ("1", 2049, 64), ("-1", 2048, 64), ("-1", 2049, 16)])
def test_wide_groups_switch_and_batch_size(monkeypatch, env, B, lpg):
    if env is not None:
        monkeypatch.setenv("EMG_WIDE_GROUPS", env)
    for fused in (True, False):
        expect(make_args(cols=64, B=B, fused=fused), 4, 1, lpg, 0)
        expect(make_args(cols=128, B=B, fused=fused, opt="sgd"), 4, 1, 64 if lpg == 64 else 32, 1)
    # a device-side step record: the launch, and with it the rule, is sized by the capacity
    a = make_args(cols=64, B=100)
    a.ctl, a.layout_B = _addr(20), B
    expect(a, 4, 1, lpg, 0)


# (optimizer, LP p, window, lr_hist) -> in-place form, on rows of 8 chunks at B = 4096 (16 lanes per group unless the form
# is compiled for a wave per group only)
IN_PLACE_FORMS = [
    ((None, 0, False, False), 0, 16),
    (("sgd", 0, False, False), 1, 16),
    (("sgd", 1, False, False), 3, 16), (("sgd", 2, False, False), 3, 16), (("sgd", 3, False, False), 3, 16),
    (("momentum", 0, False, False), 2, 16), (("momentum", 0, True, False), 4, 64),
    (("adagrad", 0, False, False), 2, 16), (("adagrad", 0, True, False), 4, 64),
    (("adam", 0, False, False), 2, 16), (("adam", 0, True, False), 5, 64),
    (("adam_lazy", 0, False, False), 2, 16), (("adam_lazy", 0, True, False), 5, 64),
    (("adam", 0, True, True), 6, 64),     # Adam's lagging singletons replayed in the kernel
    (("sgd", 2, False, True), 7, 64),     # SGD + LP, lagging singletons replayed in the kernel
]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("wide_env", [None, "0"])
def test_in_place_forms(monkeypatch, model, wide_env):
    """forms 4 to 7 are a wave per group whatever EMG_WIDE_GROUPS says"""
    if wide_env is not None:
        monkeypatch.setenv("EMG_WIDE_GROUPS", wide_env)
    for (opt, lp, window, lr_hist), ip, lpg in IN_PLACE_FORMS:
        expect(make_args(model, 32, opt=opt, lp=lp, window=window, lr_hist=lr_hist), 4, 1, lpg, ip)
        if ip <= 3:   # the same from external dL/dscore; and on scalar rows but for the LP form
            expect(make_args(model, 32, fused=False, opt=opt, lp=lp), 4, 1, lpg, ip)
            if ip != 3:
                expect(make_args(model, 30, opt=opt), 1, 1, 64, ip)
                expect(make_args(model, 30, fused=False, opt=opt), 1, 1, 64, ip)
    # the widest rows of each
    expect(make_args(model, 256, opt="adam", window=True), 4, 1, 64, 5)
    expect(make_args(model, 256, opt="adam", window=True, lr_hist=True), 4, 1, 64, 6)
    expect(make_args(model, 512, opt="sgd", lp=2, lr_hist=True), 4, 2, 64, 7)
    expect(make_args(model, 512, opt="sgd", lp=2), 4, 2, 64, 3)
    expect(make_args(model, 512, opt="adam"), 4, 2, 64, 2)


GIB_TABLE = 1 << 20        # entities of 256 columns: 1 GiB, past the Infinity Cache
SMALL_TABLE = 1000


@pytest.mark.parametrize("env,n_ent,taken", [(None, SMALL_TABLE, False), (None, GIB_TABLE, True), ("0", GIB_TABLE, False),
                                             ("1", SMALL_TABLE, True), ("1", GIB_TABLE, True)])
def test_cache_policy_form(monkeypatch, env, n_ent, taken):
    if env is not None:
        monkeypatch.setenv("EMG_CACHE_POLICY", env)
    cp = CACHE_POLICY if taken else 0
    expect(make_args(cols=256, opt="sgd", n_ent=n_ent), 4, 1, 64, 1, cp)
    expect(make_args(cols=256, opt="sgd", n_ent=n_ent, link=L.LINK_TANH), 4, 1, 64, 1, cp | LINKED)
    expect(make_args(cols=64, B=2048, opt="sgd", n_ent=n_ent if env else SMALL_TABLE), 4, 1, 64, 1, CACHE_POLICY if env == "1" else 0)
    # only plain SGD in place, at one chunk per lane of a whole wave
    expect(make_args(cols=128, opt="sgd", n_ent=n_ent), 4, 1, 32, 1)
    expect(make_args(cols=260, opt="sgd", n_ent=n_ent), 4, 2, 64, 1)
    expect(make_args(cols=256, n_ent=n_ent), 4, 1, 64, 0)
    expect(make_args(cols=256, opt="sgd", lp=2, n_ent=n_ent), 4, 1, 64, 3)
    expect(make_args(cols=256, opt="adam", n_ent=n_ent), 4, 1, 64, 2)
    expect(make_args(cols=256, fused=False, opt="sgd", n_ent=n_ent), 4, 1, 64, 1)
    expect(make_args(cols=254, opt="sgd", n_ent=n_ent), 1, 4, 64, 1)


def test_cache_policy_by_the_size_of_the_working_set():
    """unset: taken when the table is past the Infinity Cache and the rows touched twice stay within the resident budget"""
    expect(make_args(cols=256, opt="sgd", n_ent=(1 << 18)), 4, 1, 64, 1, 0)                 # 256 MiB: the table itself fits
    expect(make_args(cols=256, opt="sgd", n_ent=(1 << 18) + 1), 4, 1, 64, 1, CACHE_POLICY)
    # 5 B contribution rows of 1 KiB alone pass 240 MB from B = 46 875 on
    expect(make_args(cols=256, B=40000, eta=0, opt="sgd", n_ent=GIB_TABLE), 4, 1, 64, 1, CACHE_POLICY)
    expect(make_args(cols=256, B=50000, eta=0, opt="sgd", n_ent=GIB_TABLE), 4, 1, 64, 1, 0)


@pytest.mark.parametrize("model", MODELS)
def test_linked_forms(model):
    for kw in ({"link": L.LINK_TANH}, {"link": L.LINK_SIGMOID}, {"link": L.LINK_SOFTPLUS}, {"edge_w": True},
               {"link": L.LINK_TANH, "edge_w": True}):
        expect(make_args(model, 32, **kw), 4, 1, 16, 0, LINKED)
        expect(make_args(model, 32, opt="adam", window=True, **kw), 4, 1, 64, 5, LINKED)
        expect(make_args(model, 30, opt="sgd", **kw), 1, 1, 64, 1, LINKED)
    expect(make_args(model, 32), 4, 1, 16, 0, 0)


def test_riders_ride_the_fused_16_byte_row_kernels_only():
    expect(make_args(cols=32), 4, 1, 16, 0, 0, riders=0)
    expect(make_args(cols=32), 4, 1, 16, 0, RIDE, riders=1)
    expect(make_args(cols=512, opt="adam"), 4, 2, 64, 2, RIDE, riders=1)
    expect(make_args(cols=32, link=L.LINK_TANH), 4, 1, 16, 0, RIDE | LINKED, riders=1)
    expect(make_args(cols=30), 1, 1, 64, 0, ALONE, riders=1)
    expect(make_args(cols=32, fused=False), 4, 1, 16, 0, ALONE, riders=1)
    expect(make_args(cols=1300, fused=False), 4, 2, 64, 0, ALONE, 3, riders=1)


def test_wide_rows_run_in_blocks_of_512_columns_from_external_gradients():
    """(the shape reported is the full blocks'; the narrower last block takes its own from the same ladder at the launch)"""
    for model in MODELS:
        bw = model == L.TRANSE_L2   # (its gradient needs the full norm)
        expect(make_args(model, 513, fused=False, bw_scores=bw), 1, 8, 64, 0, 0, 2)
        expect(make_args(model, 1300, fused=False, bw_scores=bw), 4, 2, 64, 0, 0, 3)
        expect(make_args(model, 1028, B=2048, fused=False, bw_scores=bw), 4, 2, 64, 0, 0, 3)
        expect(make_args(model, 1024, fused=False, bw_scores=bw, opt="sgd", lp=3), 4, 2, 64, 3, 0, 2)
        expect(make_args(model, 512, fused=False), 4, 2, 64, 0, 0, 1)
    rc, err, _ = form(make_args(L.TRANSE_L2, 513, fused=False))
    assert rc == EINVAL and "TransE-L2 rows wider than 512 columns need bw_scores_pos" in err
    a = make_args(L.TRANSE_L2, 513, fused=False, bw_scores=True)
    a.bw_scores_neg = 0
    assert form(a)[0] == EINVAL
    a.eta, a.g_neg = 0, 0
    assert form(a)[0] == 0


def _set(**kw):
    def change(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return change


def _hyper(i, v):
    def change(a):
        a.hyper[i] = v
    return change


# (arguments, change, code, fragment of the message): every refusal on the way to the launch
REFUSALS = [
    ({}, _set(ent=0), EINVAL, "emg_train_backward_ex: null pointer"),
    ({}, _set(contrib_rel=0), EINVAL, "emg_train_backward_ex: null pointer"),
    ({}, _set(codes=0), EINVAL, "eta>0 needs codes"),
    ({}, _set(ldc=31), EINVAL, "ldc < k_int"),
    ({}, _set(fused_loss=L.LOSS_SELF_ADVERSARIAL), EINVAL, "is not pair-local"),
    ({}, _set(loss_accum=0), EINVAL, "fused loss needs loss_accum"),
    ({}, _set(bw_scores_pos=_addr(10)), EINVAL, "fused loss cannot take bw_scores"),
    ({}, _set(link=4), EINVAL, "unknown link 4"),
    ({"fused": False}, _set(link=L.LINK_TANH), EINVAL, "go through emg_link_scores and emg_link_grads"),
    ({"fused": False}, _set(edge_w=_addr(7)), EINVAL, "go through emg_link_scores and emg_link_grads"),
    ({"fused": False}, _set(g_pos=0), EINVAL, "external dL/dscore missing"),
    ({"fused": False}, _set(g_neg=0), EINVAL, "external dL/dscore missing"),
    ({}, _set(model=L.TRANSE_P), EINVAL, "EMG_TRANSE_P trains through"),
    ({"fused": False, "opt": "sgd"}, _set(model=L.TRANSE_P), EINVAL, "EMG_TRANSE_P trains through"),
    ({"fused": False}, _set(model=L.TRANSE_P, scale=0.0), EINVAL, "the order of the norm"),
    ({}, _set(loss_slots=3), EINVAL, "loss_slots must be 0 or a power of two"),
    ({}, _set(loss_slots=8192), EINVAL, "loss_slots must be 0 or a power of two"),
    ({"model": L.TRANSE_L1}, _set(fac_ws_ent=_addr(18), fac_ws_ent_bytes=1 << 30), EINVAL, "factored contributions need a bilinear model"),
    ({"opt": "sgd"}, _set(opt=5), EINVAL, "unknown optimizer"),
    ({"opt": "momentum"}, _set(ent_state0=0), EINVAL, "optimizer needs ent_state0"),
    ({"opt": "adam"}, _set(ent_state1=0), EINVAL, "adam needs both state tables"),
    ({"opt": "adam", "lp": 2}, None, EINVAL, "fold an LP regulariser for plain SGD"),
    ({"opt": "sgd", "lp": 2}, _set(lp_accum=0), EINVAL, "needs lp_accum, p in {1, 2, 3} and the tag array"),
    ({"opt": "sgd", "lp": 2}, _hyper(7, 4.0), EINVAL, "needs lp_accum, p in {1, 2, 3} and the tag array"),
    ({"opt": "sgd", "lp": 2}, _set(tag_ent=0), EINVAL, "needs lp_accum, p in {1, 2, 3} and the tag array"),
    ({"opt": "sgd", "lr_hist": True}, None, EINVAL, "lr_hist with EMG_OPT_SGD is for the fused kernel"),
    ({"opt": "sgd", "lp": 2, "lr_hist": True, "fused": False}, None, EINVAL, "lr_hist with EMG_OPT_SGD is for the fused kernel"),
    ({"opt": "sgd", "lp": 2, "lr_hist": True}, _set(step=0), EINVAL, "lr_hist with EMG_OPT_SGD is for the fused kernel"),
    ({"opt": "sgd", "lp": 2, "lr_hist": True}, _set(ctl=_addr(20), layout_B=4096), EINVAL, "lr_hist with EMG_OPT_SGD is for the fused kernel"),
    ({"opt": "sgd", "lp": 2, "lr_hist": True, "cols": 516}, None, EINVAL, "lr_hist needs 16-byte rows of at most 128 chunks"),
    ({"opt": "sgd", "lp": 2, "lr_hist": True, "cols": 30}, None, EINVAL, "lr_hist needs 16-byte rows of at most 128 chunks"),
    ({"opt": "sgd", "lp": 2, "lr_hist": True, "misaligned": True}, None, EINVAL, "lr_hist needs 16-byte rows of at most 128 chunks"),
    ({"opt": "sgd", "lp": 2, "lr_hist": True}, _set(ld_ent=33), EINVAL, "lr_hist needs 16-byte rows of at most 128 chunks"),
    ({"opt": "adam", "lr_hist": True}, None, EINVAL, "lr_hist (lagging singletons) is for the fused kernel with in-place EMG_OPT_ADAM"),
    ({"opt": "adam_lazy", "window": True, "lr_hist": True}, None, EINVAL, "lr_hist (lagging singletons) is for the fused kernel"),
    ({"opt": "momentum", "window": True, "lr_hist": True}, None, EINVAL, "lr_hist (lagging singletons) is for the fused kernel"),
    ({"opt": "adam", "window": True, "lr_hist": True, "cols": 260}, None, EINVAL, "lr_hist needs 16-byte rows of at most 64 chunks"),
    ({"opt": "adam", "window": True, "lr_hist": True, "cols": 30}, None, EINVAL, "lr_hist needs 16-byte rows of at most 64 chunks"),
    ({"opt": "adam", "window": True, "lr_hist": True}, _set(ent_state1=_addr(15, 8)), EINVAL, "and no device-side step record"),
    ({"opt": "adam", "window": True, "lr_hist": True}, _set(ctl=_addr(20), layout_B=4096), EINVAL, "and no device-side step record"),
    ({}, _set(layout_B=4095), EINVAL, "layout_B < B"),
    ({}, _set(ctl=_addr(20)), EINVAL, "a device-side step record needs layout_B"),
    ({}, _set(model=7), EINVAL, "unknown model id 7"),
    ({}, _set(model=-1), EINVAL, "unknown model id -1"),
    ({"model": L.COMPLEX}, _set(k_int=63, ldc=64), EINVAL, "bad k_int 63 for model 3"),
    ({}, _set(k_int=0), EINVAL, "bad k_int 0"),
    ({}, _set(ld_rel=31), EINVAL, "row stride smaller than k_int"),
    ({}, _set(B=-1), EINVAL, "negative sizes"),
    ({}, _set(eta=-1), EINVAL, "negative sizes"),
    ({}, _set(B=1 << 29), EINVAL, "batch too large"),
    ({"opt": "sgd", "lp": 2, "cols": 30}, None, ENOSUP, "fold an LP regulariser for 16-byte aligned rows only"),
    ({"opt": "sgd", "lp": 2, "misaligned": True}, None, ENOSUP, "fold an LP regulariser for 16-byte aligned rows only"),
    ({"opt": "sgd", "lp": 2, "fused": False, "cols": 30}, None, ENOSUP, "fold an LP regulariser for 16-byte aligned rows only"),
    ({"opt": "sgd", "window": True}, None, ENOSUP, "inplace_window (a stateful optimizer's state rows travelling with the table rows) needs"),
    ({"opt": "adam", "window": True, "fused": False}, None, ENOSUP, "fused kernel on 16-byte aligned rows of at most 64 chunks"),
    ({"opt": "adam", "window": True, "cols": 260}, None, ENOSUP, "fused kernel on 16-byte aligned rows of at most 64 chunks"),
    ({"opt": "adam", "window": True, "cols": 30}, None, ENOSUP, "fused kernel on 16-byte aligned rows of at most 64 chunks"),
    ({"opt": "adagrad", "window": True}, _set(ent_state0=_addr(14, 4)), ENOSUP, "fused kernel on 16-byte aligned rows of at most 64 chunks"),
    ({"cols": 516}, None, ENOSUP, "rows of k_int=516 are wider than the register-tiled kernel holds (512 columns per half)"),
    ({"cols": 513, "model": L.HOLE, "opt": "sgd"}, None, ENOSUP, "rows of k_int=1026 are wider than the register-tiled kernel holds"),
    ({"cols": 516, "fused": False, "model": L.TRANSE_L2}, None, EINVAL, "TransE-L2 rows wider than 512 columns need bw_scores_pos"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals(case):
    kw, change, code, fragment = REFUSALS[case]
    a = make_args(**kw)
    if change:
        change(a)
    for riders in (0, 1):   # (the same refusal with and without riders)
        rc, err, _ = form(a, riders)
        assert rc == code and fragment in err, (rc, err)


def test_null_arguments_and_empty_batches():
    lib = L.load()
    out = (C.c_int32 * 8)()
    assert lib.emg_train_backward_form(None, 0, out) == EINVAL and b"null args" in lib.emg_last_error()
    assert lib.emg_train_backward_form(C.byref(make_args()), 0, None) == EINVAL
    a = make_args()
    a.B, a.ent = 0, 0            # an empty batch is no error and no scoring launch, whatever else the arguments say; riders go alone
    assert lib.emg_train_backward_form(C.byref(a), 0, out) == 0 and list(out) == [0] * 8
    assert lib.emg_train_backward_form(C.byref(a), 1, out) == 0 and list(out) == [0, 0, 0, 0, 0, 0, ALONE, 0]
    a = make_args(fused=False)   # any order of the norm: generic kernels, riders alone
    a.model = L.TRANSE_P
    assert lib.emg_train_backward_form(C.byref(a), 1, out) == 0 and list(out) == [PASS_BACKWARD, L.TRANSE_P, 0, 0, 0, 0, ALONE, 0]


SWEEP = [dict(fused=fused, opt=opt, lp=lp, window=window, lr_hist=lr_hist, link=link, misaligned=mis)
         for fused in (True, False)
         for opt, lp, window, lr_hist in ((None, 0, False, False), ("sgd", 0, False, False), ("sgd", 2, False, False), ("sgd", 3, False, True),
                                          ("momentum", 0, False, False), ("adagrad", 0, True, False), ("adam", 0, True, False),
                                          ("adam", 0, True, True))
         for link in (L.LINK_LINEAR, L.LINK_SIGMOID)
         for mis in (False, True)
         if fused or (link == L.LINK_LINEAR and not lr_hist)]


@pytest.mark.parametrize("model", MODELS)
def test_every_width_gets_a_kernel_or_a_refusal(model):
    """columns 1 .. 2100 (per half for complex models) under every combination above: the dry run looks the kernel of the decided
    form up, so success means there is one; a refusal is one of the documented ones, never a form without a kernel"""
    lib = L.load()
    out = (C.c_int32 * 8)()
    cplx = model in (L.COMPLEX, L.HOLE)
    bw = model == L.TRANSE_L2
    forms = set()
    for kw in SWEEP:
        a = make_args(model, 4, bw_scores=bw and not kw["fused"], **kw)
        ref = C.byref(a)
        for cols in range(1, 2101):
            a.k_int = a.ld_ent = a.ld_rel = a.ldc = 2 * cols if cplx else cols
            rc = lib.emg_train_backward_form(ref, cols & 1, out)
            if rc == 0:
                W, NV, LPG, ip, flags, blocks = out[2:8]
                assert W in (1, 4) and NV in (1, 2, 4, 8) and LPG in (16, 32, 64) and blocks == (cols + 511) // 512
                assert blocks == 1 or not kw["fused"]
                assert (W == 4) == (cols % 4 == 0 and not kw["misaligned"])
                assert ip < 4 or (LPG == 64 and W == 4 and kw["fused"])
                assert bool(flags & LINKED) == (kw["link"] != L.LINK_LINEAR)
                forms.add((W, NV, LPG, ip, flags & 3))
            else:
                assert rc in (EINVAL, ENOSUP)
                err = lib.emg_last_error()
                assert err and b"no kernel for" not in err, (cols, kw, err)
    assert len(forms) > 20


def test_the_set_of_training_kernels():
    """no training-step kernel added, dropped or renamed: the library's kernels against the recorded names"""
    from tests.test_host_logic import _device_kernels_of_the_library
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "train_kernel_names.txt"), encoding="ascii") as f:
        recorded = f.read().split()
    built = sorted(s for s, _, _ in _device_kernels_of_the_library() if s.startswith("_ZN3emg") and "train_" in s)
    assert built == recorded
