"""Host-side network model (gym_anm_amd/model.py): the one-time setup of Simulator.__init__.

* known answers of the reference's own tests, restated as data
  (tests/simulator/test_simulator_basics.py:35-46, 69-174; test_network_checks.py; test_bus.py;
  test_branch.py; test_devices.py spec errors);
* every constant against what the reference's Simulator objects hold for several networks and for 400
  mutated ones (bit-exact), recorded in tests/golden/reference_constants.npz by oracle/make_golden_constants.py."""
import os

import numpy as np
import numpy.testing as npt
import pytest

from gym_anm_amd import errors as E
from gym_anm_amd import networks
from gym_anm_amd.model import NetworkModel

from conftest import GOLDEN

_N = None


def basics_network():
    return {
        "baseMVA": 10,
        "bus": np.array([[0, 1, 50, 1.1, 0.9], [2, 1, 50, 1.1, 0.9], [1, 0, 100, 1.0, 1.0]]),
        "branch": np.array([[0, 1, 0.1, 0.2, 0.3, 20, 1, 90], [1, 2, 0.4, 0.5, 0.6, 20, 2, 0]]),
        "device": np.array(
            [
                [1, 0, -1, 0.2, 0, -10, _N, _N, _N, _N, _N, _N, _N, _N, _N],
                [0, 1, 0, _N, 200, -200, 200, -200, _N, _N, _N, _N, _N, _N, _N],
                [2, 2, 2, _N, 30, 0, 30, -30, _N, _N, _N, _N, _N, _N, _N],
                [3, 2, 3, _N, 50, -50, 50, -50, _N, _N, _N, _N, 100, 0, 0.9],
            ],
            dtype=object,
        ),
    }


def test_ordering_and_counts():
    m = NetworkModel(basics_network(), 1, 100, require_solvable=False)
    assert m.bus_ids == [0, 1, 2] and m.branch_ids == [(0, 1), (1, 2)] and m.dev_ids == [0, 1, 2, 3]
    assert (m.N_bus, m.N_device, m.N_load, m.N_non_slack_gen, m.N_des) == (3, 4, 1, 1, 1)


def test_bus_bounds_and_spaces():
    base = 10
    m = NetworkModel(basics_network(), 1, 100, require_solvable=False)
    npt.assert_array_equal(m.bus_p_min, np.array([-10, -200, -50]) / base)
    npt.assert_array_equal(m.bus_p_max, np.array([0, 200, 80]) / base)
    npt.assert_array_equal(m.bus_q_min, np.array([-2, -200, -80]) / base)
    npt.assert_array_equal(m.bus_q_max, np.array([0, 200, 80]) / base)
    lo, hi = m.action_bounds()
    npt.assert_array_equal(lo, [0, -30, -50, -50])
    npt.assert_array_equal(hi, [30, 30, 50, 50])
    sb = m.state_bounds()
    assert sb["bus_v_magn"][1] == {"pu": (1.0, 1.0), "kV": (100.0, 100.0)}
    assert sb["bus_v_ang"][1] == {"degree": (0, 0), "rad": (0, 0)}
    assert sb["bus_v_magn"][0]["pu"] == (-np.inf, np.inf)
    assert sb["dev_p"][2] == {"MW": (0.0, 30.0), "pu": (0.0, 3.0)}
    assert sb["dev_q"][1] == {"MVAr": (-2.0, 0.0), "pu": (-0.2, 0.0)}
    assert sb["des_soc"][3] == {"MWh": (0.0, 100.0), "pu": (0.0, 10.0)}
    assert sb["gen_p_max"][2] == {"MW": (0.0, 30.0), "pu": (0.0, 3.0)}
    assert sb["branch_s"][(0, 1)]["MVA"] == (-np.inf, np.inf)


def test_solver_assumptions_are_enforced_for_the_gpu_path():
    with pytest.raises(E.UnsupportedNetworkError, match="slack"):
        NetworkModel(basics_network(), 1, 100)
    net = networks.two_bus_network()
    net["bus"] = np.array([[0, 0, 50, 1.0, 1.0], [2, 1, 50, 1.1, 0.9]])
    net["branch"] = np.array([[0, 2, 0.01, 0.1, 0.0, 32, 1, 0]])
    net["device"][1][1] = 2
    with pytest.raises(E.UnsupportedNetworkError, match="bus IDs"):
        NetworkModel(net, 1, 100)


def _two(dev_row=None, bus=None, branch=None, base=100):
    net = {
        "baseMVA": base,
        "bus": np.array([[0, 0, 50, 1.0, 1.0], [1, 1, 100, 1.1, 0.9]]) if bus is None else bus,
        "branch": np.array([[0, 1, 0.1, 0.2, 0.3, 20, 1, 0]]) if branch is None else branch,
        "device": np.array(
            [
                [0, 0, 0, _N, 200, -200, 200, -200, _N, _N, _N, _N, _N, _N, _N],
                [1, 1, -1, 0.2, 0, -10, _N, _N, _N, _N, _N, _N, _N, _N, _N] if dev_row is None else dev_row,
            ],
            dtype=object,
        ),
    }
    return net


@pytest.mark.parametrize("base", [-1, 0])
def test_base_mva_error(base):
    with pytest.raises(E.BaseMVAError):
        NetworkModel(_two(base=base), 1, 100)


def test_network_level_errors():
    with pytest.raises(E.BusSpecError):  # duplicate bus ids
        NetworkModel(_two(bus=np.array([[0, 0, 50, 1.0, 1.0], [1, 1, 100, 1.1, 0.9], [1, 1, 100, 1.1, 0.9]])), 1, 100)
    with pytest.raises(E.BusSpecError):  # no slack bus
        NetworkModel(_two(bus=np.array([[0, 1, 50, 1.0, 1.0], [1, 1, 100, 1.1, 0.9]])), 1, 100)
    with pytest.raises(E.BranchSpecError):  # parallel branches
        NetworkModel(_two(branch=np.array([[0, 1, 0.1, 0.2, 0.3, 20, 1, 0], [1, 0, 0.1, 0.2, 0.3, 20, 1, 0]])), 1, 100)
    with pytest.raises(E.BranchSpecError):  # branch to a missing bus
        NetworkModel(_two(branch=np.array([[0, 3, 0.1, 0.2, 0.3, 20, 1, 0]])), 1, 100)
    net = _two()
    net["device"][1][0] = 0  # duplicate device id
    with pytest.raises(E.DeviceSpecError):
        NetworkModel(net, 1, 100)
    net = _two()
    net["device"][0][1] = 1  # slack device not on the slack bus
    with pytest.raises(E.DeviceSpecError):
        NetworkModel(net, 1, 100)


@pytest.mark.parametrize(
    "row,err",
    [
        ([1, 1, -1, _N, 0, -10, _N, _N, _N, _N, _N, _N, _N, _N, _N], E.LoadSpecError),  # load without Q/P
        ([1, 1, -1, 0.2, 5, -10, _N, _N, _N, _N, _N, _N, _N, _N, _N], E.LoadSpecError),  # load with P_max > 0
        ([1, 1, 2, _N, -5, 0, 30, -30, _N, _N, _N, _N, _N, _N, _N], E.GenSpecError),  # PMAX < 0
        ([1, 1, 2, _N, 5, 10, 30, -30, _N, _N, _N, _N, _N, _N, _N], E.GenSpecError),  # PMAX < PMIN
        ([1, 1, 2, _N, 30, 0, 30, -30, 40, _N, _N, _N, _N, _N, _N], E.GenSpecError),  # P+ > PMAX
        ([1, 1, 2, _N, 30, 0, 30, -30, 20, _N, 40, _N, _N, _N, _N], E.GenSpecError),  # Q+ > QMAX
        ([1, 1, 3, _N, 50, -50, 50, -50, _N, _N, _N, _N, _N, 0, 0.9], E.StorageSpecError),  # no SOC_MAX
        ([1, 1, 3, _N, 50, -50, 50, -50, _N, _N, _N, _N, 100, 0, 1.5], E.StorageSpecError),  # EFF > 1
        ([1, 1, 3, _N, 50, 10, 50, -50, _N, _N, _N, _N, 100, 0, 0.9], E.StorageSpecError),  # PMIN > 0
        ([1, 5, -1, 0.2, 0, -10, _N, _N, _N, _N, _N, _N, _N, _N, _N], E.DeviceSpecError),  # unknown bus
        ([1, 1, 7, 0.2, 0, -10, _N, _N, _N, _N, _N, _N, _N, _N, _N], NotImplementedError),  # unknown type (simulator.py:173-174)
        ([1, 1, 1.5, 0.2, 30, 0, 30, -30, _N, _N, _N, _N, _N, _N, _N], E.DeviceSpecError),  # non-integer type (devices.py:85-88)
    ],
)
def test_device_spec_errors(row, err):
    with pytest.raises(err):
        NetworkModel(_two(dev_row=row), 1, 100)


@pytest.mark.parametrize(
    "branch",
    [[0, 1, -0.1, 0.2, 0.3, 20, 1, 0], [0, 1, 0.0, 0.0, 0.3, 20, 1, 0], [0, 1, 0.1, 0.2, 0.3, -2, 1, 0],
     [0, 1, 0.1, 0.2, 0.3, 20, 0, 0], [0, 1, 0.1, 0.2, 0.3, 20, 1, 400]],
)  # fmt: skip
def test_branch_spec_errors(branch):
    with pytest.raises(E.BranchSpecError):
        NetworkModel(_two(branch=np.array([branch])), 1, 100)


@pytest.mark.parametrize("bus_row", [[1, 3, 100, 1.1, 0.9], [1, 1, -5, 1.1, 0.9], [1, 1, 100, 0.8, 0.9]])
def test_bus_spec_errors(bus_row):
    with pytest.raises(E.BusSpecError):
        NetworkModel(_two(bus=np.array([[0, 0, 50, 1.0, 1.0], bus_row])), 1, 100)


def test_defaults_and_flex_constants():
    # tau/rho of the ANM6 devices in the reference's expression order
    m = NetworkModel(networks.anm6_network(), 0.25, 100)
    k = m.dev_ids.index(2)
    assert m.dev_tau[k, 0] == (0.15 - 0.3) / (0.3 - 0.2) and m.dev_tau[k, 1] == (-0.15 - -0.3) / (0.3 - 0.2)
    assert m.dev_rho[k, 0] == 0.3 - m.dev_tau[k, 0] * 0.2
    k = m.dev_ids.index(6)
    npt.assert_allclose(m.dev_tau[k], [-1.25, 1.25, -1.25, 1.25], rtol=1e-12)
    npt.assert_allclose(m.dev_rho[k], [0.875, -0.875, -0.875, 0.875], rtol=1e-12)
    assert m.dev_soc_max[k] == 1.0 and m.dev_eff[k] == 0.9
    # defaults: unrated branch, missing limits
    net = _two(dev_row=[1, 1, 2, _N, _N, _N, _N, _N, _N, _N, _N, _N, _N, _N, _N],
               branch=np.array([[0, 1, 0.1, 0.2, _N, _N, _N, _N]], dtype=object))  # fmt: skip
    m = NetworkModel(net, 1, 100)
    assert m.br_rate[0] == np.inf and m.br_tap[0] == 1.0 and m.br_shunt[0] == 0
    assert m.dev_p_max[1] == np.inf and m.dev_p_min[1] == 0.0 and m.dev_q_min[1] == -np.inf


def _reference_constants():
    """tests/golden/reference_constants.npz (oracle/make_golden_constants.py): what the reference's Simulator made of
    the stock networks and of the mutated ones"""
    with np.load(os.path.join(GOLDEN, "reference_constants.npz")) as z:
        return {k: z[k] for k in z.files}


def _recorded(z, case):
    """the fields of one stock network `case` of `_reference_constants()`"""
    r = {k[len(case) + 1:]: v for k, v in z.items() if k.startswith(case + "/")}
    assert r, "no case %s in reference_constants.npz" % case
    return r


def _recorded_mutations(z):
    """(the exception class each of the 400 mutated networks raised in the reference, "" where it was accepted; the
    fields of every accepted network, in order)"""
    lens = {k[len("mutations/"):-len("_len")]: v for k, v in z.items() if k.startswith("mutations/") and k.endswith("_len")}
    n = {len(v) for v in lens.values()}
    assert len(n) == 1, "packed fields of different network counts: %r" % n
    ends = {k: np.concatenate(([0], np.cumsum(v))) for k, v in lens.items()}
    accepted = [{k: z["mutations/" + k][e[j]:e[j + 1]] for k, e in ends.items()} for j in range(n.pop())]
    return z["mutations/exception"].tolist(), accepted


def _assert_same_constants(m, r):
    """`m` against the reference's recorded constants `r` (`_recorded`)"""
    import ast

    def eq(x, y):  # bit-equal, NaN == NaN (what a degenerate but accepted spec yields on both sides)
        return x == y or (x != x and y != y)

    npt.assert_array_equal(m.Y_bus, r["Y_bus"])
    assert m.bus_ids == r["bus_ids"].tolist() and m.dev_ids == r["dev_ids"].tolist()
    assert m.branch_ids == [tuple(b) for b in r["branch_ids"].tolist()]
    for k, kind in enumerate(r["dev_kind"].tolist()):
        for a, b in ((m.dev_p_min[k], r["dev_p_min"][k]), (m.dev_p_max[k], r["dev_p_max"][k]), (m.dev_q_min[k], r["dev_q_min"][k]),
                     (m.dev_q_max[k], r["dev_q_max"][k])):
            assert eq(a, b)
        if kind in (1, 2):  # generator, storage unit
            assert eq(m.dev_tau[k, 0], r["tau"][k, 0]) and eq(m.dev_tau[k, 1], r["tau"][k, 1])
            assert eq(m.dev_rho[k, 0], r["rho"][k, 0]) and eq(m.dev_rho[k, 1], r["rho"][k, 1])
        if kind == 2:  # storage unit
            assert eq(m.dev_tau[k, 2], r["tau"][k, 2]) and eq(m.dev_tau[k, 3], r["tau"][k, 3])
            assert eq(m.dev_rho[k, 2], r["rho"][k, 2]) and eq(m.dev_rho[k, 3], r["rho"][k, 3])
            assert (m.dev_soc_min[k], m.dev_soc_max[k], m.dev_eff[k]) == tuple(r["soc"][k])
    for k in range(len(r["br_rate"])):
        assert (m.br_series[k] == r["br_series"][k] and m.br_shunt[k] == r["br_shunt"][k] and m.br_tap[k] == r["br_tap"][k]
                and m.br_rate[k] == r["br_rate"][k])
    # nested bounds dictionaries (the reference's state_bounds, recorded flat in its own order)
    rb = {q: {} for q in r["sb_quantities"].tolist()}
    for q, i in r["sb_ids"].tolist():
        rb[q][ast.literal_eval(i)] = {}
    for (q, i, unit), (lo, hi) in zip(r["sb_units"].tolist(), r["sb_lohi"].tolist()):
        rb[q][ast.literal_eval(i)][unit] = (lo, hi)
    mb = m.state_bounds()
    assert set(rb) == set(mb)
    for q in rb:
        assert list(rb[q].keys()) == list(mb[q].keys()), q
        for i in rb[q]:
            for unit, (lo, hi) in rb[q][i].items():
                assert eq(mb[q][i][unit][0], lo) and eq(mb[q][i][unit][1], hi), (q, i, unit)
    lo, hi = m.action_bounds()
    npt.assert_array_equal(lo, r["act_lo"])
    npt.assert_array_equal(hi, r["act_hi"])


def stock_networks():
    return {
        "anm6": networks.anm6_network(),
        "basics": basics_network(),
        "3bus_tx": networks.three_bus_loop_network(1.0437, 23.1),
        "case30": networks.synthetic_radial_network(30, 0),
        "2bus": networks.two_bus_network(),
    }


@pytest.mark.parametrize("which", ["anm6", "basics", "3bus_tx", "case30", "2bus"])
def test_constants_bit_identical_to_reference(which):
    m = NetworkModel(stock_networks()[which], 0.25, 100, require_solvable=False)
    _assert_same_constants(m, _recorded(_reference_constants(), which))


BUILTIN_CRASHES = ("TypeError", "KeyError", "IndexError", "ValueError", "AttributeError", "ZeroDivisionError", "UnboundLocalError")


def _mutations(rng, n):
    """Malformed (and a few still-valid) variants of the 3-bus / 5-device basics network: one random field of one
    random row replaced by a value of a random kind (missing, zero, negative, huge, swapped sign, duplicate id)."""
    import copy

    base = basics_network()
    for _ in range(n):
        net = copy.deepcopy({k: (np.array(v, dtype=object) if isinstance(v, np.ndarray) else v) for k, v in base.items()})
        what = rng.choice(["bus", "branch", "device", "device", "device", "baseMVA", "drop"])
        if what == "baseMVA":
            net["baseMVA"] = rng.choice([0, -1, 10, None])
        elif what == "drop":
            tab = rng.choice(["bus", "branch", "device"])
            r = rng.integers(len(net[tab]))
            net[tab] = np.delete(net[tab], r, axis=0)
        else:
            tab = net[what]
            r, c = rng.integers(tab.shape[0]), rng.integers(tab.shape[1])
            old = tab[r, c]
            kind = rng.choice(["none", "zero", "neg", "big", "flip", "dup", "small"])
            tab[r, c] = {"none": None, "zero": 0, "neg": -abs(old) - 1 if old is not None else -1, "big": 1e4,
                         "flip": (-old if old is not None else 1), "dup": tab[(r + 1) % tab.shape[0], c],
                         "small": 1e-3}[kind]
        yield net


def test_front_end_agrees_with_the_reference_on_mutated_networks():
    """Differential test of the network-dict front end: 400 random single-field mutations of a
    valid network, against what the reference's Simulator made of each (tests/golden/reference_constants.npz,
    oracle/make_golden_constants.py); both must accept or both must raise, with the same exception class
    (check_network.py:7-64, components/*.py); accepted networks give bit-identical Y_bus, device limits, tau / rho,
    storage constants, branch constants, state bounds and action box."""
    ref_excs, ref_accepted = _recorded_mutations(_reference_constants())
    assert len(ref_excs) == 400 and ref_excs.count("") == len(ref_accepted), "stale reference_constants.npz"
    rng = np.random.default_rng(12)
    n_ok = n_err = 0
    for i, net in enumerate(_mutations(rng, 400)):
        ref_exc, got_exc = ref_excs[i] or None, None
        ref = ref_accepted[ref_excs[:i].count("")] if ref_exc is None else None   # the reference's constants of this network
        try:
            m = NetworkModel(net, 0.25, 100, require_solvable=False)
        except Exception as ex:  # noqa: BLE001
            got_exc = type(ex).__name__
        shown = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in net.items()}
        if ref_exc in BUILTIN_CRASHES:
            # the reference trips over the garbage before any of its checks (a TypeError from comparing None, an
            # IndexError from a dropped row ...): no error class to agree on, but the network must not be accepted
            assert got_exc is not None, (ref_exc, shown)
            n_err += 1
            continue
        if ref_exc is None and got_exc == "BusSpecError" and any(r[1] == 0 and r[4] is None for r in net["bus"]):
            n_err += 1  # deliberate: a slack bus without VMIN passes the reference's constructor and crashes its first step
            continue
        assert ref_exc == got_exc, (ref_exc, got_exc, shown)
        if ref_exc is None:
            n_ok += 1
            _assert_same_constants(m, ref)
        else:
            n_err += 1
    assert n_ok > 40 and n_err > 100, (n_ok, n_err)
