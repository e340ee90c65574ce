"""GPU: runtime.capture_graph — the one warm-up / restore / capture / restore helper every captured pass of the package goes
through.  With `state` the warm-ups are undone and each replay advances the state once; without, the warm-ups stand."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _counter_step():
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.zeros(1, dtype=torch.int32, device=DEV)

    def step():
        counter.add_(1)
        out.copy_(counter)
        return out

    return counter, out, step


@pytest.mark.parametrize("warmups", [1, 2])
def test_capture_graph_restores_its_state(warmups):
    from teal_amd import runtime
    counter, out, step = _counter_step()
    g, value = runtime.capture_graph(step, state=[counter], warmups=warmups)
    assert value is out and int(counter) == 0
    for _ in range(3):
        g.replay()
    assert int(counter) == 3 and int(out) == 3


@pytest.mark.parametrize("warmups", [1, 2])
def test_capture_graph_without_state_undoes_nothing(warmups):
    """Nothing is put back: every step that ran stands.  The warm-ups run; the capturing call of step() is recorded into the
    graph and not executed (measured on an MI355X: the counter reads 1 and 2 behind the call at warmups 1 and 2, not 2 and 3),
    so the counter reads `warmups` behind the call and the first replay is the first run of the captured step."""
    from teal_amd import runtime
    counter, out, step = _counter_step()
    g, _ = runtime.capture_graph(step, warmups=warmups)
    print(f"warmups {warmups}: counter {int(counter)} behind the call")
    assert int(counter) == warmups and int(out) == warmups
    g.replay()
    assert int(counter) == warmups + 1 and int(out) == warmups + 1
