"""Host side of the stream attention body: who takes attention="stream", where --attention is valid, and the argument refusals of the
two entries that return before a device is needed."""
import pytest

from teal_amd import _lib
from teal_amd.gpt_fast import engine_features as EF
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.batched import BatchedDecodeEngine, SlotDecodeEngine
from teal_amd.gpt_fast.engine import DecodeEngine
from teal_amd.gpt_fast.speculative import SpeculativeDecoder


def _args(*extra):
    return G.build_parser().parse_args(["--device", "cuda", "--synthetic", "tiny-test", *extra])


def test_the_keyword_and_who_takes_it():
    assert EF.ATTENTION_BODIES == ("chunked", "stream")
    for kind in ("slot", "batched", "decode", "speculative", "tensor-parallel"):
        assert EF.attention_refusal(kind, "chunked") is None and "unknown attention" in EF.attention_refusal(kind, "flash")
        why = EF.attention_refusal(kind, "stream")
        assert (why is None) if kind in ("slot", "batched") else (kind in why and "no second body" in why)
    for cls in (BatchedDecodeEngine, SlotDecodeEngine):  # (refused before the model is looked at)
        with pytest.raises(ValueError, match="unknown attention 'flash'"):
            cls(None, [], 2, attention="flash")
    with pytest.raises(ValueError, match="DecodeEngine.*the decode path"):
        DecodeEngine(None, [], attention="stream")

    class Sharded:
        tp_world = 2

    with pytest.raises(ValueError, match="the tensor-parallel path"):
        DecodeEngine(Sharded(), [], attention="stream")
    with pytest.raises(ValueError, match="speculative decoding.*the speculative path"):
        SpeculativeDecoder(None, None, 4, 0.8, 50, False, 64, attention="stream")


def test_the_flag_is_refused_outside_batch_size_and_requests(monkeypatch, tmp_path):
    assert _args().attention == "chunked" and G.check_attention_args(_args()) == "chunked"
    assert G.check_attention_args(_args("--attention", "stream", "--batch_size", "4")) == "stream"
    assert G.check_attention_args(_args("--attention", "stream", "--requests", str(tmp_path / "r.jsonl"))) == "stream"
    with pytest.raises(SystemExit, match=r"--attention stream.*the decode path.*needs --batch_size > 1 or --requests"):
        G.main(_args("--attention", "stream", "--compile"))
    with pytest.raises(SystemExit, match="--attention stream.*the speculative path"):
        G.check_attention_args(_args("--attention", "stream", "--self_speculate"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--attention stream.*the tensor-parallel path"):
        G.check_attention_args(_args("--attention", "stream", "--batch_size", "4"))
    assert G.check_attention_args(_args("--batch_size", "4")) == "chunked"


@pytest.mark.parametrize("kv8", [False, True], ids=["16bit", "kv8"])
def test_argument_refusals_come_before_any_device(kv8):
    L = _lib.load()
    f = L.teal_batched_decode_attention_stream_kv8 if kv8 else L.teal_batched_decode_attention_stream
    p = 0x10000  # (never dereferenced: every call below is refused on its arguments)
    caches = [p, p, p, p] if kv8 else [p, p]
    nc = len(caches)
    #        slabs split rope pos active            yt partials bytes   B  H  KV hd  S   dtype stream
    full = [p, 2, p, p, None, *caches, p, p, 1 << 20, 2, 8, 2, 64, 96, 0, None]
    for i in (0, 2, 3, *range(5, 5 + nc + 2)):  # a null pointer (active may be NULL: every slot), the scales included
        assert f(*[None if j == i else v for j, v in enumerate(full)]) == -1, i
    t = 5 + nc + 3  # the index of B
    put = lambda i, v: [v if j == i else x for j, x in enumerate(full)]  # noqa: E731
    assert f(*put(1, 0)) == -1 and f(*put(1, 17)) == -1                                          # split
    assert f(*put(t + 5, 2)) == -2                                                                # dtype
    assert f(*put(t, 0)) == -3 and f(*put(t, 9)) == -3 and f(*put(t + 3, 96)) == -3 and f(*put(t + 2, 3)) == -3 and f(*put(t + 4, 0)) == -3
    assert f(*put(0, p + 4)) == -4 and f(*put(5, p + 8)) == -4 and f(*put(6, p + 2)) == -4       # slabs, K, V off 16 bytes
