"""GPU tier: device-resident gait schedules (bpmpc_gait_batch, bpmpc_solver_setup_gaits) against bpmpc_solver_setup_commands, the host
pre-pass (bpmpc_solver_setup fed with the oracle's windows) and a restatement of the reference's loop with the oracle's GaitSchedule:
one GaitSchedule per robot, getModeSchedule(t0 - H, t0 + 2 H) at every setup, then a pending GaitReceiver command inserted at (t0 + H, H).
  node tables, node times, layout                  bit-identical (contraction is off in the device code)
  schedules after every setup                      bit-identical to the oracle's GaitSchedule
  targets / xref / initial iterate                 1e-13 (device sin / cos may differ in the last place)
  solve output x, u                                1e-9 between the two paths, 1e-8 against the oracle"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ["stance", "trot", "standing_trot", "flying_trot"]
TABLES = (("g_kind", 1), ("g_mode", 1), ("g_dt", 1), ("g_start", 1), ("g_zref", 4), ("g_zdref", 4))


@pytest.fixture(scope="module")
def ctx():
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios
    from oracle import ingest, reference_py as rp
    from tests import oracle_bridge as ob
    itf = scenarios.h1_interface()
    lib = [bp.loadModeSequenceTemplate(scenarios.H1["gait"], n) for n in NAMES]
    lib_o = [ingest.load_gait_template(scenarios.H1["gait"], n) for n in NAMES]
    return bp, scenarios, rp, ob, itf, lib, lib_o


class Fleet:
    """The reference's loop per robot, restated with the oracle's GaitSchedule (GaitSchedule.cpp:46-137, GaitReceiver.cpp:49-59)."""

    def __init__(self, ctx, n):
        bp, sc, rp, ob, itf, lib, lib_o = ctx
        m = ob.model("h1")
        self.rp, self.lib, self.bp = rp, lib_o, bp
        self.g = [rp.GaitSchedule(*m["initial_mode_schedule"], m["default_template"], m["phase_transition_stance_time"]) for _ in range(n)]
        self.ins, self.cmd = [None] * n, [None] * n

    def insert(self, b, g, start, final):
        self.ins[b] = (g, start, final)

    def command(self, b, g):
        self.cmd[b] = g

    def setup(self, t0, H, batch=None):
        windows = []
        for b in range(batch or len(self.g)):
            t = float(np.broadcast_to(t0, (len(self.g),))[b])
            if self.ins[b] is not None:
                g, s, f = self.ins[b]
                self.g[b].insert_mode_sequence_template(self.lib[g], s, f)
                self.ins[b] = None
            ev, ms = self.g[b].get_mode_schedule(t - H, t + 2 * H)
            windows.append(self.bp.ModeSchedule(np.array(ev, float), np.array(ms, np.int32)))
            if self.cmd[b] is not None:
                self.g[b].insert_mode_sequence_template(self.lib[self.cmd[b]], t + H, H)
                self.cmd[b] = None
        return windows

    def state(self, b):
        return list(self.g[b].event_times), list(self.g[b].mode_sequence)


class DeviceInts:
    """An int32 array in device memory of the library's own HIP runtime, seen through __cuda_array_interface__ (what a torch.int32 tensor
    on the GPU offers as well)."""

    def __init__(self, values):
        self.hip = C.CDLL("libamdhip64.so")
        a = np.ascontiguousarray(values, np.int32)
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(a.nbytes)) == 0
        assert self.hip.hipMemcpy(self.ptr, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0   # host to device, synchronous
        self.__cuda_array_interface__ = {"shape": a.shape, "typestr": "<i4", "data": (self.ptr.value, False), "version": 3, "strides": None}

    def free(self):                                                            # after a setup has read the commands (it synchronises)
        self.hip.hipFree(self.ptr)


def _tables(mpc, nb):
    N = mpc.max_nodes
    pg = mpc.read("p_grid").astype(int)[:nb]
    out = {name: mpc.read(name).reshape(mpc.max_batch, N, w)[pg] for name, w in TABLES}
    out["nodes"] = mpc.read("g_nodes").astype(int)[pg]
    out["g_time"] = mpc.read("g_time").reshape(mpc.max_batch, N + 1)[pg]
    out["pg"] = pg
    return out


def _same_tables(ta, tb, robots):
    for b in robots:
        assert ta["nodes"][b] == tb["nodes"][b], b
        for name in [n for n, _ in TABLES] + ["g_time"]:
            assert np.array_equal(ta[name][b], tb[name][b]), (name, b)          # whole stride, padding included


def _same_schedules(gs, fleet, robots):
    for b in robots:
        ms = gs.modeSchedule(b)
        ev, mo = fleet.state(b)
        assert list(ms.eventTimes) == ev and list(ms.modeSequence) == mo, b


def test_no_commands_equals_setup_commands(ctx):
    bp, sc, rp, ob, itf, lib, lib_o = ctx
    starts = [sc.GAIT_START, 0.0, 0.137]
    rows = [(g, s) for g in range(4) for s in starts]
    nb, H, tick = len(rows), 30 * sc.DT, 0.02
    gop, gst = np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows])
    x0 = sc.perturbed_initial_states(itf, nb)
    cmd = np.tile([0.2, 0.0, 0.0, 0.1], (nb, 1))
    ref = bp.BatchedSqpMpc(itf, max_batch=nb, max_nodes=64)
    dev = bp.BatchedSqpMpc(itf, max_batch=nb, max_nodes=64)
    gs = bp.BatchedGaitSchedule(dev, lib)
    for t_first in (0.0, 512.0):
        gs.reset()
        gs.insertModeSequenceTemplate(gop, gst, t_first + 2 * H)
        for k in range(51 if t_first == 0.0 else 3):
            t0 = t_first + k * tick
            lr = ref.setup_commands(t0, x0, lib, gop, gst, cmd, horizon=H)
            ld = dev.setup_gaits(gs, t0, x0, cmd, horizon=H)
            assert lr == ld and ld["n_grids"] == nb, (t0, lr, ld)
            _same_tables(_tables(ref, nb), _tables(dev, nb), range(nb))
            if k % 25 == 0:
                assert np.array_equal(ref.read("xref"), dev.read("xref")) and np.array_equal(ref.read("x"), dev.read("x"))


def test_gait_receiver_semantics_against_oracle(ctx):
    bp, sc, rp, ob, itf, lib, lib_o = ctx
    nb, NI, tick = 64, 30, 0.02
    H = NI * sc.DT
    fleet = Fleet(ctx, nb)
    host = bp.BatchedSqpMpc(itf, max_batch=nb, max_nodes=72)
    dev = bp.BatchedSqpMpc(itf, max_batch=nb, max_nodes=72)
    gs = bp.BatchedGaitSchedule(dev, lib)
    first = np.array([1 + b % 3 for b in range(nb)], np.int32)                # trot / standing_trot / flying_trot
    gs.insertModeSequenceTemplate(first, sc.GAIT_START, 2 * H)
    for b in range(nb):
        fleet.insert(b, int(first[b]), sc.GAIT_START, 2 * H)
    x0 = sc.perturbed_initial_states(itf, nb)
    cmd = np.array([(0.3 * np.cos(b), 0.1 * np.sin(b), 0.0, 0.2 * np.sin(3 * b)) for b in range(nb)])
    rng = np.random.default_rng(7)
    plan = {k: {} for k in range(14)}
    for b in range(nb):                                                        # scattered commands over all four gaits
        for k in rng.choice(13, size=2, replace=False):
            plan[int(k)][b] = int(rng.integers(0, 4))
    plan[2][0], plan[3][0] = 2, 3                                              # robot 0: commands on consecutive ticks
    plan[4][1] = int(first[1])                                                 # robot 1: a command to its current gait
    for k in range(14):
        t0 = k * tick
        if k == 5:                                                             # robot 2: two commands before one setup, the latest wins
            gs.command(np.array([-1, -1, 3] + [-1] * (nb - 3), np.int32))
            fleet.command(2, 3)
            plan[5][2] = 1
        for b, g in plan[k].items():
            fleet.command(b, g)
        c = np.full(nb, -1, np.int32)
        c[list(plan[k])] = list(plan[k].values())
        gs.command(c)
        windows = fleet.setup(t0, H)
        targets = [itf.cmdVelToTargetTrajectories(tuple(cmd[b]), t0, x0[b], H) for b in range(nb)]
        host.setup(t0, x0, windows, targets, horizon=H)
        dev.setup_gaits(gs, t0, x0, cmd, horizon=H)
        _same_schedules(gs, fleet, range(nb))
        th, td = _tables(host, nb), _tables(dev, nb)
        _same_tables(th, td, range(nb))
        N = dev.max_nodes
        for name, shape in (("xref", (N, dev.nx)), ("x", (N + 1, dev.nx)), ("u", (N, dev.nu))):
            a, d = host.read(name).reshape(-1, *shape)[:nb], dev.read(name).reshape(-1, *shape)[:nb]
            assert np.abs(a - d).max() < 1e-13 * max(1.0, np.abs(a).max()), name
        if k % 4 != 3:
            continue
        host.enqueue(); dev.enqueue()
        t1, x1, u1, _, s1 = host.fetch()
        t2, x2, u2, _, s2 = dev.fetch()
        assert np.array_equal(t1, t2)
        for b in range(nb):
            n = s1[b].n_nodes
            assert s2[b].n_nodes == n
            assert np.abs(x1[b, :n + 1] - x2[b, :n + 1]).max() < 1e-9 and np.abs(u1[b, :n] - u2[b, :n]).max() < 1e-9 * max(1.0, np.abs(u1[b]).max())
        if k == 11:                                                            # and against the oracle's own pre-pass + solve
            prob = dict(t0=np.full(nb, t0), x0=x0, schedule=windows, targets=targets, horizon=H)
            for b in (0, 2, 37):
                xo, uo, _, _ = ob.oracle_solve_like(prob, b)
                n = s2[b].n_nodes
                assert np.abs(x2[b, :n + 1] - xo).max() / max(1.0, np.abs(xo).max()) < 1e-8
                assert np.abs(u2[b, :n] - uo).max() / max(1.0, np.abs(uo).max()) < 1e-8


def test_recalled_preRun_order_command_shapes_the_next_window_only(ctx):
    """SolverBase::preRun [OCS2-upstream, recalled]: the reference manager's getModeSchedule runs before the GaitReceiver, so a command
    issued before setup k leaves setup k's tables unchanged; setup k + 1 differs only from t0_k + H on, behind a STANCE phase of
    phaseTransitionStanceTime (the phase there is a swing of the trot)."""
    bp, sc, rp, ob, itf, lib, lib_o = ctx
    H, tick = 30 * sc.DT, 0.02
    stance = float(itf.get("phase_transition_stance_time")[0])
    mpc = bp.BatchedSqpMpc(itf, max_batch=2, max_nodes=64)
    gs = bp.BatchedGaitSchedule(mpc, lib)
    x0 = sc.perturbed_initial_states(itf, 2)
    gs.insertModeSequenceTemplate(1, sc.GAIT_START, 2 * H)                    # both robots trot
    mpc.setup_gaits(gs, 0.0, x0, (0.2, 0, 0, 0), horizon=H)
    gs.command(np.array([3, -1], np.int32))                                    # robot 0 -> flying_trot before setup k
    tk = tick
    lay = mpc.setup_gaits(gs, tk, x0, (0.2, 0, 0, 0), horizon=H)
    assert lay["n_grids"] == 2                                                 # histories differ from here on ...
    t = _tables(mpc, 2)
    _same_tables({k: v[[0]] for k, v in t.items()}, {k: v[[1]] for k, v in t.items()}, [0])   # ... but setup k's tables do not
    mpc.setup_gaits(gs, tk + tick, x0, (0.2, 0, 0, 0), horizon=H)
    s0, s1 = gs.modeSchedule(0), gs.modeSchedule(1)
    cut = tk + H
    before0, before1 = s0.eventTimes[s0.eventTimes < cut], s1.eventTimes[s1.eventTimes < cut]
    assert np.array_equal(before0, before1) and np.array_equal(s0.modeSequence[:len(before0) + 1][:-1], s1.modeSequence[:len(before1)])
    i = len(before0)
    assert s1.modeSequence[i] != 3                                             # the trot swings at t0_k + H ...
    assert s0.eventTimes[i] == cut and s0.modeSequence[i + 1] == 3 and s0.eventTimes[i + 1] == cut + stance   # ... robot 0 stands first
    assert list(s0.modeSequence[i + 2:i + 6]) == [1, 0, 2, 0]                  # then flies
    t = _tables(mpc, 2)                                                        # setup k + 1's grids agree in front of t0_k + H
    n0, n1 = (int(np.searchsorted(t["g_time"][r][:t["nodes"][r] + 1], cut)) for r in (0, 1))
    assert n0 == n1 and np.array_equal(t["g_time"][0][:n0], t["g_time"][1][:n0]) and np.array_equal(t["g_mode"][0][:n0 - 1], t["g_mode"][1][:n0 - 1])
    assert t["g_time"][0][n0] == cut and t["g_kind"][0][n0] == 1                # robot 0's grid has the event at t0_k + H


def test_grid_sharing(ctx):
    bp, sc, rp, ob, itf, lib, lib_o = ctx
    nb, H, tick = 256, 30 * sc.DT, 0.02
    mpc = bp.BatchedSqpMpc(itf, max_batch=nb, max_nodes=64)
    gs = bp.BatchedGaitSchedule(mpc, lib)
    x0 = sc.perturbed_initial_states(itf, nb)
    gs.insertModeSequenceTemplate(1, sc.GAIT_START, 2 * H)
    for k in range(3):
        assert mpc.setup_gaits(gs, k * tick, x0, (0.2, 0, 0, 0), horizon=H)["n_grids"] == 1
    plan = {3: {5: 2, 77: 3}, 4: {200: 2}}                                    # robots 5 and 200: the same command one tick apart
    for k in range(3, 9):
        c = np.full(nb, -1, np.int32)
        for b, g in plan.get(k, {}).items():
            c[b] = g
        gs.command(c)
        lay = mpc.setup_gaits(gs, k * tick, x0, (0.2, 0, 0, 0), horizon=H)
        pg = mpc.read("p_grid").astype(int)[:nb]
        distinct = 1 + (k >= 3) * 2 + (k >= 4)
        assert lay["n_grids"] == distinct == len(set(pg)), (k, lay)
        if k >= 4:
            assert pg[5] != pg[200]


def test_device_commands_equal_host_commands(ctx):
    bp, sc, rp, ob, itf, lib, lib_o = ctx
    nb, H, tick = 16, 30 * sc.DT, 0.02
    mpc = bp.BatchedSqpMpc(itf, max_batch=nb, max_nodes=72)
    ga, gb = bp.BatchedGaitSchedule(mpc, lib), bp.BatchedGaitSchedule(mpc, lib)
    x0 = sc.perturbed_initial_states(itf, nb)
    for g in (ga, gb):
        g.insertModeSequenceTemplate(np.arange(nb, dtype=np.int32) % 3 + 1, sc.GAIT_START, 2 * H)
    rng = np.random.default_rng(3)
    for k in range(8):
        c = np.where(rng.random(nb) < 0.3, rng.integers(0, 4, nb), -1).astype(np.int32)
        ga.command(c)
        dc = DeviceInts(c)
        gb.command(dc)
        if k == 2:                                                             # a host command behind a device one: the latest wins
            ga.command(np.array([0] + [-1] * (nb - 1), np.int32)); gb.command(np.array([0] + [-1] * (nb - 1), np.int32))
        la = mpc.setup_gaits(ga, k * tick, x0, (0.2, 0, 0, 0), horizon=H)
        ta = _tables(mpc, nb)
        lb = mpc.setup_gaits(gb, k * tick, x0, (0.2, 0, 0, 0), horizon=H)
        dc.free()
        tb = _tables(mpc, nb)
        assert la == lb
        _same_tables(ta, tb, range(nb))
        for b in range(nb):
            sa, sb = ga.modeSchedule(b), gb.modeSchedule(b)
            assert np.array_equal(sa.eventTimes, sb.eventTimes) and np.array_equal(sa.modeSequence, sb.modeSequence)


def test_rejected_setup_changes_nothing_and_reset_equals_a_fresh_handle(ctx):
    bp, sc, rp, ob, itf, lib, lib_o = ctx
    nb, H, tick = 8, 30 * sc.DT, 0.02
    fast = bp.ModeSequenceTemplate(np.array([0.0, 0.01, 0.02]), np.array([1, 2], np.int32))
    fast_o = ([0.0, 0.01, 0.02], [1, 2])
    mpc = bp.BatchedSqpMpc(itf, max_batch=nb, max_nodes=48)
    gs = bp.BatchedGaitSchedule(mpc, lib + [fast])
    fleet = Fleet(ctx, nb)
    fleet.lib = lib_o + [fast_o]
    x0 = sc.perturbed_initial_states(itf, nb)
    gs.insertModeSequenceTemplate(1, sc.GAIT_START, 2 * H)
    for b in range(nb):
        fleet.insert(b, 1, sc.GAIT_START, 2 * H)

    def setup(t0):
        fleet.setup(t0, H)
        return mpc.setup_gaits(gs, t0, x0, (0.2, 0, 0, 0), horizon=H)

    setup(0.0)
    gs.command(np.array([-1, -1, -1, 4, -1, -1, -1, -1], np.int32)); fleet.command(3, 4)   # robot 3 -> 10 ms phases, after setup 0.02
    setup(tick)
    before = [gs.modeSchedule(b) for b in range(nb)]
    gs.command(np.array([-1, -1, -1, -1, -1, 2, -1, -1], np.int32))           # pending for robot 5 across the rejected calls
    with pytest.raises(bp.BpmpcError) as e:                                   # the 10 ms phases are inside this window: too many nodes
        mpc.setup_gaits(gs, tick + 0.6, x0, (0.2, 0, 0, 0), horizon=H)
    assert e.value.status == -6 and "max_nodes" in str(e.value)
    bad = DeviceInts([-1, 9] + [-1] * (nb - 2))
    gs.command(bad)                                                            # an unknown template, noticed by the next setup
    with pytest.raises(bp.BpmpcError) as e:
        mpc.setup_gaits(gs, 2 * tick, x0, (0.2, 0, 0, 0), horizon=H)
    assert e.value.status == -1
    bad.free()
    for b in range(nb):
        after = gs.modeSchedule(b)
        assert np.array_equal(after.eventTimes, before[b].eventTimes) and np.array_equal(after.modeSequence, before[b].modeSequence), b
    gs.command(np.array([-1, 1] + [-1] * (nb - 2), np.int32))                 # the latest command replaces the bad one
    fleet.command(5, 2); fleet.command(1, 1)
    lay = setup(2 * tick)
    assert lay["batch"] == nb
    _same_schedules(gs, fleet, range(nb))
    setup(3 * tick)
    _same_schedules(gs, fleet, range(nb))                                      # robot 5's command survived both rejected calls
    assert gs.modeSchedule(5).modeSequence.tolist() != gs.modeSchedule(6).modeSequence.tolist()
    gs.reset()
    fresh = bp.BatchedGaitSchedule(mpc, lib + [fast])
    for b in range(nb):
        a, f = gs.modeSchedule(b), fresh.modeSchedule(b)
        assert np.array_equal(a.eventTimes, f.eventTimes) and np.array_equal(a.modeSequence, f.modeSequence)
    for g in (gs, fresh):
        g.insertModeSequenceTemplate(2, sc.GAIT_START, 2 * H)
    la = mpc.setup_gaits(gs, 0.5, x0, (0.2, 0, 0, 0), horizon=H)
    ta = _tables(mpc, nb)
    lf = mpc.setup_gaits(fresh, 0.5, x0, (0.2, 0, 0, 0), horizon=H)
    assert la == lf and la["n_grids"] == 1
    _same_tables(ta, _tables(mpc, nb), range(nb))


def test_closed_loop_with_gait_switches(ctx):
    bp, sc, rp, ob, itf, lib, lib_o = ctx
    nb, NI, tick, ticks = 256, 67, 0.02, 300                                  # the reference's own horizon, as tools/closed_loop_soak.py
    H = NI * sc.DT
    mpc = bp.BatchedSqpMpc(itf, max_batch=nb, max_nodes=sc.max_nodes_for(NI, H), return_gains=True)
    gs = bp.BatchedGaitSchedule(mpc, lib)
    fleet = Fleet(ctx, nb)
    gs.insertModeSequenceTemplate(1, sc.GAIT_START, 2 * H)
    for b in range(nb):
        fleet.insert(b, 1, sc.GAIT_START, 2 * H)
    switches = {}                                                              # robot -> {tick: gait}: two switches each, at its own ticks
    for b in range(nb):
        k1 = 10 + (b * 7) % 120
        k2 = k1 + 40 + (b * 13) % 100
        switches[b] = {k1: 2 if b % 2 else 3, k2: 1}
    cmd = np.array([(0.2 + 0.1 * np.sin(b), 0.05 * np.cos(b), 0.0, 0.1 * np.sin(2 * b)) for b in range(nb)])
    x0 = sc.perturbed_initial_states(itf, nb)
    fleet.setup(0.0, H)
    mpc.setup_gaits(gs, 0.0, x0, cmd, horizon=H)
    mpc.enqueue()
    for k in range(1, ticks + 1):
        c = np.full(nb, -1, np.int32)
        for b in range(nb):
            if k in switches[b]:
                c[b] = switches[b][k]
                fleet.command(b, switches[b][k])
        gs.command(c)
        mpc.rollout(tick, fetch=False)
        fleet.setup(k * tick, H)
        mpc.setup_gaits(gs, k * tick, None, cmd, horizon=H, from_previous=True)
        mpc.enqueue()
    _, x, _, _, st = mpc.fetch()
    assert all(s.status == 0 for s in st[:nb])
    assert np.isfinite(x[:nb]).all()
    _same_schedules(gs, fleet, range(nb))
