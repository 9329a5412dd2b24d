"""CPU test of NavierStokes_Component's opt-in reverse mode (sem_amd/solvers/components.py) around a solver double:
the oracle's NS solver (tests/oracle_solvers.py) with _get_dresiduals_T / _get_update_T from the dense matrix of its own
dresiduals, so the component's wiring -- which bar goes where, accumulation into the entries that are present, absent
entries, the temperature bar asked for only when T_cd is present, the iteration count, the default's errors -- is
checked where no GPU exists.  The d_inputs['T_cd'] path (transfer_T runs on the device) and the device solver are
covered by tests/test_gpu_ns_adjoint.py."""
import numpy as np
import pytest

OUT = ("u_ns", "v_ns", "p_ns")


def _double():
    from oracle_solvers import OracleCD, OracleNS

    class NS(OracleNS):
        calls = []

        def _matrix(self):
            N = self.N
            cols = [np.hstack(self.o.dresiduals(*np.split(e, 3))) for e in np.eye(3 * N)]
            return np.stack(cols, axis=1)

        def _get_dresiduals_T(self, ru_bar, rv_bar, rc_bar, want_T=False):
            self.calls.append(("dres_T", want_T))
            y = self._matrix().T @ np.hstack((ru_bar, rv_bar, rc_bar))
            return tuple(np.split(y, 3))

        def _get_update_T(self, du_bar, dv_bar, dp_bar, dres_c0=None):
            self.calls.append(("update_T", None if dres_c0 is None else np.array(dres_c0)))
            lam = np.linalg.solve(self._matrix().T, np.hstack((du_bar, dv_bar, dp_bar)))
            return tuple(np.split(lam, 3))

    ns = NS(1.0, 1.0, 50.0, 20.0, 3, 3, 3)      # odd x odd elements: the Jacobian is regular
    cd = OracleCD(1.0, 1.0, 30.0, 2, 2, 3, T_W=0.5, T_E=-0.5)
    return ns, cd


def _linearised(adjoint):
    from sem_amd.solvers.components import NavierStokes_Component
    ns, cd = _double()
    c = NavierStokes_Component(solver_NS=ns, solver_CD=cd, **({"adjoint": True} if adjoint else {}))
    c.setup()
    rng = np.random.default_rng(8)
    inp = {"T_cd": rng.uniform(-1, 1, cd.N)}
    out = {n: 0.1 * rng.uniform(-1, 1, ns.N) for n in OUT}
    c.apply_nonlinear(inp, out, {})
    c.linearize(inp, out, None)
    return c, ns, cd, inp, out, rng


def test_reverse_mode_wiring():
    c, ns, cd, inp, out, rng = _linearised(True)
    assert c.options["adjoint"] is True
    N = ns.N
    w = {n: rng.uniform(-1, 1, N) for n in OUT}
    pre = {n: rng.uniform(-1, 1, N) for n in OUT}
    want = dict(zip(OUT, ns._get_dresiduals_T(*(w[n] for n in OUT))))
    ns.calls.clear()
    dout = {n: pre[n].copy() for n in OUT}
    c.apply_linear(inp, out, {}, dout, dict(w), "rev")
    assert ns.calls == [("dres_T", False)]          # no T_cd in d_inputs: the temperature bar is not computed
    for n in OUT:
        assert np.array_equal(dout[n], pre[n] + want[n]), n
    # absent d_outputs entries are skipped, absent d_residuals entries count as zero
    dout = {"p_ns": pre["p_ns"].copy()}
    c.apply_linear(inp, out, {}, dout, {"v_ns": w["v_ns"]}, "rev")
    assert list(dout) == ["p_ns"]
    z = np.zeros(N)
    assert np.array_equal(dout["p_ns"], pre["p_ns"] + ns._get_dresiduals_T(z, w["v_ns"], z)[2])
    # the dot identity against forward mode (dT = 0)
    d = {n: rng.uniform(-1, 1, N) for n in OUT}
    dres = {}
    c.apply_linear(inp, out, {"T_cd": np.zeros(cd.N)}, dict(d), dres, "fwd")
    lhs, rhs = sum(np.dot(dres[n], w[n]) for n in OUT), sum(np.dot(d[n], want[n]) for n in OUT)
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    # solve_linear('rev'): d_residuals = A^-T d_outputs, d_residuals['p_ns'] the initial guess when present
    b = {n: rng.uniform(-1, 1, N) for n in OUT}
    guess = rng.uniform(-1, 1, N)
    ns.calls.clear()
    before = c.iter_count_solve
    dres = {"p_ns": guess.copy()}
    c.solve_linear(dict(b), dres, "rev")
    assert c.iter_count_solve == before + 1 and set(dres) == set(OUT)
    assert ns.calls[0][0] == "update_T" and np.array_equal(ns.calls[0][1], guess)
    back = ns._get_dresiduals_T(*(dres[n] for n in OUT))
    for n, a in zip(OUT, back):
        assert np.abs(a - b[n]).max() <= 1e-9
    ns.calls.clear()
    c.solve_linear(dict(b), {}, "rev")
    assert ns.calls[0][1] is None


def test_default_stays_forward_only():
    c, ns, cd, inp, out, rng = _linearised(False)
    assert c.options["adjoint"] is False
    z = {n: np.zeros(ns.N) for n in OUT}
    with pytest.raises(ValueError, match="only forward mode implemented"):
        c.apply_linear(inp, out, {"T_cd": np.zeros(cd.N)}, dict(z), dict(z), "rev")
    with pytest.raises(ValueError, match="only forward mode implemented"):
        c.solve_linear(dict(z), dict(z), "rev")
    assert ns.calls == []
