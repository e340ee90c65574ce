"""What the feature benches (logprobs_bench.py, logit_processors_bench.py, sampling_bench.py, stop_bench.py) share: the command
line, the record, the synthetic model and its engines, and the timing of hipGraph replays with HIP events."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from teal_amd import runtime  # noqa: E402
from teal_amd.gpt_fast import generate as G  # noqa: E402


def replay_ms(g, steps, reset):
    """ms per replay over `steps` replays from the state reset() restores, after 3 warm replays from the same state"""
    reset()
    for _ in range(3):
        g.replay()
    reset()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with runtime.graph_capture(g):
        fn()
    return g


class FeatureBench:
    """One run of a feature bench: parses the command line (`settings`: the script's own, comma-separated, as the default of
    --settings), prints the record's head line (`head`: the script's own keys, in front of the note) and collects every line."""

    def __init__(self, settings: str, note_eg: str = "which tree this is", **head):
        p = argparse.ArgumentParser()
        p.add_argument("--synthetic", default="7B")
        p.add_argument("--precision", default="fp16", choices=["fp16", "bf16"])
        p.add_argument("--sparsity", type=float, default=0.5)
        p.add_argument("--n_layer", type=int, default=None)
        p.add_argument("--steps", type=int, default=200)
        p.add_argument("--pos", type=int, default=32, help="position of the first timed step")
        p.add_argument("--chain", type=int, default=20, help="leg 3: launches per graph")
        p.add_argument("--legs", default="1,2,3")
        p.add_argument("--settings", default=settings)
        p.add_argument("--note", default="", help=f"a line for the head of the record (e.g. {note_eg})")
        p.add_argument("--out", default=None, help="also append the record to this file")
        self.a = a = p.parse_args()
        runtime.init()
        self.dev, self.dt = "cuda", {"fp16": torch.float16, "bf16": torch.bfloat16}[a.precision]
        self.legs, self.settings = a.legs.split(","), a.settings.split(",")
        self.max_seq = a.pos + a.steps + 16
        self.lines = []
        self.emit({"model": a.synthetic, "n_layer": a.n_layer, "precision": a.precision, "sparsity": a.sparsity, "steps": a.steps,
                   "pos": a.pos, "chain": a.chain, "device": torch.cuda.get_device_name(0), **head, "note": a.note})

    def emit(self, rec):
        line = json.dumps(rec)
        print(line, flush=True)
        self.lines.append(line)

    def rounds(self):
        """every setting twice, alternating: the spread between a setting's two runs is the noise a difference has to beat"""
        return [(rnd, key) for rnd in (1, 2) for key in self.settings]

    def model(self):
        """(model, thresholds, the eight prompts of pos - s tokens: slots admitted on them sit at different positions)"""
        a = self.a
        m = G.build_synthetic_model(a.synthetic, self.dev, self.dt, n_layer=a.n_layer)
        ths = G.apply_sparsity(m, sparsity=a.sparsity, hist_path=None, greedy_lookup=None, synthetic=True)
        V = m.config.vocab_size
        return m, ths, [torch.randint(0, V, (a.pos - s,), generator=torch.Generator().manual_seed(s)).tolist() for s in range(8)]

    def caches(self, m, B):
        m.max_seq_length, m.max_batch_size = -1, -1
        m.setup_caches(max_batch_size=B, max_seq_length=self.max_seq)

    def decode_engine(self, m, ths):
        """a DecodeEngine about to take the step at --pos, and the state a timed window starts from"""
        from teal_amd.gpt_fast.engine import DecodeEngine
        self.caches(m, 1)
        eng = DecodeEngine(m, ths)
        g = torch.Generator(device=self.dev).manual_seed(0)
        eng.tok_buf.copy_(torch.randint(0, m.config.vocab_size, (1, 1), device=self.dev, generator=g))
        eng.pos_buf.fill_(self.a.pos)
        eng.rng_state.copy_(torch.tensor([1234, 0], dtype=torch.int64))
        return eng, [eng.tok_buf, eng.pos_buf, eng.rng_state]

    def slot_engine(self, m, ths, prompts, B=8):
        """a SlotDecodeEngine with every slot admitted (none retires inside a window), and the state a timed window starts from"""
        from teal_amd.gpt_fast.batched import SlotDecodeEngine
        self.caches(m, B)
        eng = SlotDecodeEngine(m, ths, B)
        for s in range(B):
            eng.admit(s, prompts[s], self.max_seq, None, 1234 + s)
        return eng, [eng.tok_buf, eng.pos_buf, eng.rng_state, eng.slot_state]

    def close(self):
        if self.a.out:
            os.makedirs(os.path.dirname(os.path.abspath(self.a.out)), exist_ok=True)
            with open(self.a.out, "a") as f:
                f.write("\n".join(self.lines) + "\n")
