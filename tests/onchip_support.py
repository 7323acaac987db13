"""What the on-chip GPU test files share (tests/test_gpu_onchip*.py, test_gpu_steps_many.py, test_gpu_wave_many.py): the cap of the
on-chip plan, a system created whatever MI355CG_ONCHIP says, the parameters of a batch or ensemble call and the result fields the
files compare.  A plain module: no test in here.  Each file keeps its own pairs of systems: a handle carries workspaces and state."""
import os

DOMAIN = (1.0, 2.0, 1.0, 2.0)
FIELDS = ("iterations", "stop_reason", "converged", "r_norm2", "initial_r_norm2", "final_precision", "final_residual_norm")


def cap():
    import iterative_solvers_amd as isa
    cap = 64
    while True:                                   # the largest n mi355cg_onchip_plan accepts
        try:
            isa.onchip_plan(cap + 2)
        except ValueError:
            return cap
        cap += 2


def system(n, onchip=False, domain=DOMAIN):
    import iterative_solvers_amd as isa
    old = os.environ.pop("MI355CG_ONCHIP", None)
    try:
        s = isa.MatrixFreeSystem(n, n, *domain)
    finally:
        if old is not None:
            os.environ["MI355CG_ONCHIP"] = old
    if onchip:
        s.set_solve_mode(isa.SOLVE_ONCHIP)
    assert s.solve_mode_info()["mode"] == (isa.SOLVE_ONCHIP if onchip else isa.SOLVE_LAUNCHES)
    return s


def params(rule, **kw):
    """the parameters the batch and ensemble entry points take: no true solution"""
    import iterative_solvers_amd as isa
    p = isa.default_params(rule)
    p.use_true_solution = 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def fields(res):
    return tuple(getattr(res, f) for f in FIELDS)
