"""CPU: runs.py -- the kernel sequence AlternatingSolver.issue enqueues for every kind of solver
(the literals are the sequences of the run driver as it stood in qmc.py), the eager fallback of
run(), the graph chunks, the one cost rule to the bit, and that a solver which provides nothing
but c_step / s_step goes through the driver.  No device."""
import ast
import math
import os

import pytest
import torch

from quantized_spectrum_cartography_amd import runs
from quantized_spectrum_cartography_amd.runs import AlternatingSolver, cost_history, graph_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, S, B, L, F = "c_step", "s_step", "fused_body", "fused_last", "c_finish"


class Recorder(AlternatingSolver):
    """Every hook and step appends its name to `log`."""

    def __init__(self, fuse=False, chain=False, ahead=False):
        super().__init__()
        self.fuse, self.chain, self._is_ahead = fuse, chain, ahead
        self.C = torch.zeros(1)
        self.log = []

    def begin_run(self):
        self.log.append("begin_run")

    def ahead(self):
        return self._is_ahead

    def c_step(self):
        self.log.append(C)

    def s_step(self):
        self.log.append(S)

    def fused_body(self):
        self.log.append(B)

    def fused_last(self):
        self.log.append(L)

    def c_finish(self):
        self.log.append(F)


PLAIN = {0: [], 1: [C, S], 2: [C, S, C, S], 3: [C, S, C, S, C, S]}
SEQUENCES = [
    (dict(), PLAIN),
    (dict(chain=True), PLAIN),  # (chain without fuse: no fused launch to end a run with)
    (dict(fuse=True), {0: [], 1: [C, S], 2: [C, B, S], 3: [C, B, B, S]}),
    (dict(fuse=True, chain=True), {0: [], 1: [C, L], 2: [C, B, L], 3: [C, B, B, L]}),
    (dict(fuse=True, chain=True, ahead=True), {0: [], 1: [F, L], 2: [F, B, L], 3: [F, B, B, L]}),
]


@pytest.mark.parametrize("kw,expected", SEQUENCES)
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_issue_order(kw, expected, n):
    sol = Recorder(**kw)
    sol.issue(n)
    assert sol.log == ["begin_run"] + expected[n]


@pytest.mark.parametrize("kw,expected", SEQUENCES)
def test_run_with_use_graph_off_the_gpu_issues_eagerly(kw, expected):
    for n in range(4):
        a, b = Recorder(**kw), Recorder(**kw)
        a.issue(n)
        b.run(n, use_graph=True)  # (C is a host tensor: nothing to capture)
        assert b.log == a.log == ["begin_run"] + expected[n]
        assert b._graphs == {}


@pytest.mark.parametrize("m", [1, 4, 1024])
def test_graph_chunks(m):
    assert graph_chunks(0, m) == []
    assert graph_chunks(2 * m + 1, m) == [m, m, 1]
    for n in (1, m - 1, m, m + 1, 3 * m, 5 * m + 3):
        ch = graph_chunks(n, m)
        assert sum(ch) == n and all(0 < c <= m for c in ch)
    assert graph_chunks(2049) == [1024, 1024, 1] and runs.GRAPH_MAX_ITERS == 1024


ROWS = [[0.1, 0.2, 0.3, 0.09], [1.1, 2.2, 0.03, 1e-3], [3.3, 0.4, 0.9, 0.6]]
NSQ_FINAL, LC, LS = 0.07, 0.3, 0.1


def test_cost_history_one_term_to_the_bit():
    """The sharded solvers' form: nll + lambda_c sqrt(.) + lambda_s sqrt(nsq_s)."""
    cc, cs = cost_history(ROWS, NSQ_FINAL, LC, [(LS * math.sqrt(r[3]),) for r in ROWS])
    for i, (nll_c, nll_s, nsq_c, nsq_s) in enumerate(ROWS):
        nsq_c_next = ROWS[i + 1][2] if i + 1 < len(ROWS) else NSQ_FINAL
        assert cc[i] == nll_c + LC * math.sqrt(nsq_c) + LS * math.sqrt(nsq_s)
        assert cs[i] == nll_s + LC * math.sqrt(nsq_c_next) + LS * math.sqrt(nsq_s)
    assert len(cc) == len(cs) == 3
    assert cs[2] == 0.4 + LC * math.sqrt(NSQ_FINAL) + LS * math.sqrt(0.6)  # the last row


def test_cost_history_two_terms_left_to_right():
    """Free S with a prior: ((nll + lambda_c sqrt(.)) + lambda_s sqrt(nsq_s)) + prior, and 0.0
    for an absent prior changes nothing."""
    prior = [0.2, 0.3, 0.0]
    cc, cs = cost_history(ROWS, NSQ_FINAL, LC,
                          [(LS * math.sqrt(r[3]), prior[i]) for i, r in enumerate(ROWS)])
    for i, (nll_c, nll_s, nsq_c, nsq_s) in enumerate(ROWS):
        nsq_c_next = ROWS[i + 1][2] if i + 1 < len(ROWS) else NSQ_FINAL
        assert cc[i] == nll_c + LC * math.sqrt(nsq_c) + LS * math.sqrt(nsq_s) + prior[i]
        assert cs[i] == nll_s + LC * math.sqrt(nsq_c_next) + LS * math.sqrt(nsq_s) + prior[i]
    # the order is visible in fp64 with these values: another association gives another number
    a, b, c = 0.1 + LC * math.sqrt(0.3), LS * math.sqrt(0.09), 0.2
    assert (a + b) + c != a + (b + c) and cc[0] == (a + b) + c
    one = cost_history(ROWS, NSQ_FINAL, LC, [(LS * math.sqrt(r[3]),) for r in ROWS])
    assert (cc[2], cs[2]) == (one[0][2], one[1][2])
    assert cost_history([], NSQ_FINAL, LC, []) == ([], [])


def test_a_solver_with_only_the_two_steps_runs():
    class Minimal(AlternatingSolver):
        C = torch.zeros(1)

        def c_step(self):
            self.n_c = vars(self).get("n_c", 0) + 1

        def s_step(self):
            self.n_s = vars(self).get("n_s", 0) + 1

    sol = Minimal()
    sol.issue(2)
    sol.prepare(5)
    sol.run(3)
    sol.run(1, use_graph=True)
    assert (sol.n_c, sol.n_s) == (6, 6) and sol._graphs == {}
    assert (sol.fuse, sol.chain, sol.dist, sol.graph_tolerant, sol.graph_capturable,
            sol.graph_error, sol.graph_iters, sol.graph_pool, sol.graph_state) == \
        (False, False, None, False, True, None, runs.GRAPH_MAX_ITERS, None, ())
    with pytest.raises(NotImplementedError):
        AlternatingSolver().issue(1)


def test_runs_imports_nothing_of_the_package_and_qmc_reexports_it():
    tree = ast.parse(open(os.path.join(ROOT, "quantized_spectrum_cartography_amd", "runs.py")).read())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            assert node.level == 0, "relative import in runs.py"
            mods.add(node.module)
        elif isinstance(node, ast.Import):
            mods.update(a.name for a in node.names)
    assert mods <= {"ctypes", "math", "time", "warnings", "torch"}
    from quantized_spectrum_cartography_amd import qmc
    for n in ("capture_stream", "quiesce_collectives", "stream_capture_status", "abandon_capture",
              "graph_chunks", "GRAPH_MAX_ITERS"):
        assert getattr(qmc, n) is getattr(runs, n), n
    assert qmc.GEN_GRAPH_ITERS == qmc.GeneratorSolver.graph_iters == 32
