"""Continuous batching: requests of different prompt lengths and budgets share the B <= 8 slots of one batched step.

A request is prompt token ids, a token budget and an optional EOS id.  The step (SlotDecodeEngine, teal_amd/gpt_fast/batched.py)
switches a finished slot off on the device, so a captured step replays unchanged whatever the active set; TEAL's rule stays
per sequence and a step reads the union of the rows the ACTIVE sequences keep.  Between bursts of `sync_every` replays the
host reads the slot state back in one copy, harvests the finished requests (their history rows) and admits waiting ones in FIFO
order, one dense prompt pass each.

refill="free" admits into every free slot; refill="all" only when every slot is free — static batching on the same engine
(the benchmark's baseline).  Request r draws from its own stream, seed + r (draw 0 is its first token, draw i decode step i),
so its tokens do not depend on its slot, on the requests beside it or on sync_every (where the union does not either: every
row kept).

What a request may carry beyond that — a shared prefix, logprobs, logit processors, its own sampling, stop conditions, a constraint,
its own sparsity, forced tokens — is one object each (Prefixes ... Forced below; ContinuousBatcher.features): the batcher's defaults, what
is refused before anything runs, whether the engine feature is switched on, the keywords of the request's admission, and what the
result gains.  A new per-request feature is one more such object; the scheduling loop names none of them.
"""
from __future__ import annotations

import json
import math
import time
from collections import deque
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

from .batched import SLOT_ACTIVE, SLOT_FINISH, SLOT_PRODUCED, SLOT_STEP
from .constraints import MAX_TEMPERATURE, Automaton
from .logit_processors import fp32
from .stopping import MAX_IDS, MAX_SEQ_LEN, MAX_SEQS

REFILL = ("free", "all")
SAMPLING = ("temperature", "top_k", "top_p", "min_p")
MAX_LEVELS = 8  # distinct sparsity levels of one run: each is resolved to thresholds before anything runs


@dataclass
class Request:
    tokens: List[int]
    max_new_tokens: int
    eos_id: Optional[int] = None
    seed: Optional[int] = None  # its random stream; None: the batcher's seed + its index
    prefix: Optional[str] = None  # a shared prefix's id: `tokens` are the suffix after its rows
    # logit processors (None: the batcher's default).  In order of application: a positive logit of every prompt or generated token is
    # divided by repetition_penalty, any other multiplied; frequency_penalty times the count of its generations and presence_penalty
    # (once) are subtracted from a generated token's logit; logit_bias {"<id>": value} is added
    repetition_penalty: Optional[float] = None
    presence_penalty: Optional[float] = None
    frequency_penalty: Optional[float] = None
    logit_bias: Optional[Dict[str, float]] = None
    # sampling (None: the batcher's default).  In order of application: temperature, top_k (0: off), top_p over the renormalised
    # top-k set (1: off), min_p relative to the most likely token (0: off)
    temperature: Optional[float] = None
    top_k: Optional[int] = None
    top_p: Optional[float] = None
    min_p: Optional[float] = None
    # stop conditions (None: the batcher's default; stop sequences have none).  The request ends right after one of the ids, or after
    # the last token of one of the sequences (up to 8 of up to 8 token ids, matched against what it generated only); nothing but
    # its budget and the cache end stops it before min_new_tokens tokens.  The stopping tokens stay in its output
    stop_token_ids: Optional[List[int]] = None
    stop_sequences: Optional[List[List[int]]] = None
    min_new_tokens: Optional[int] = None
    # constrained decoding, at most one of the three: the id of a registered automaton; token-id lists of which the request produces
    # exactly one, then its EOS id (it needs one); token ids the request draws all its tokens from
    constraint: Optional[str] = None
    choices: Optional[List[List[int]]] = None
    allowed_token_ids: Optional[List[int]] = None
    # its own sparsity level in [0, 1) (None: the run's): the thresholds its slot keeps rows under
    sparsity: Optional[float] = None
    # teacher forcing: token ids its draws 0 .. n-1 yield in place of what the sampler drew (n <= max_new_tokens; with n ==
    # max_new_tokens the request only scores them, with a larger budget it goes on sampling behind them: an answer prefix).  A
    # forced token is a drawn token for every rule that follows — EOS, stop conditions, budget, processors
    forced_tokens: Optional[List[int]] = None

    def __post_init__(self):
        if sum(v is not None for v in (self.constraint, self.choices, self.allowed_token_ids)) > 1:
            raise ValueError("a request takes at most one of constraint, choices and allowed_token_ids")
        if self.forced_tokens is not None:
            if not _token_ids(self.forced_tokens):
                raise ValueError("forced_tokens must be a non-empty list of token ids")
            if any(v is not None for v in (self.constraint, self.choices, self.allowed_token_ids)):
                raise ValueError("forced_tokens do not combine with constraint, choices or allowed_token_ids: a forced token may be one "
                                 "the automaton bans")
            if len(self.forced_tokens) > self.max_new_tokens:
                raise ValueError(f"{len(self.forced_tokens)} forced_tokens exceed max_new_tokens {self.max_new_tokens}")

    def constraint_spec(self):
        """None, or (name, automaton): the automaton built from `choices` / `allowed_token_ids` under a name made of its content
        (equal lists share one image), or (constraint, None) for a registered one"""
        if self.constraint is not None:
            return self.constraint, None
        if self.choices is not None:
            Automaton.from_choices(self.choices)  # (refuses what is no list of token id lists)
            canon = sorted({tuple(c) for c in self.choices})  # the set decides, not the order or a repeat
            return "choices:" + json.dumps(canon, separators=(",", ":")), Automaton.from_choices(canon)
        if self.allowed_token_ids is not None:
            a = Automaton.from_allowed(self.allowed_token_ids)
            return "allowed:" + json.dumps([t for t, _ in a.states[0]["edges"]], separators=(",", ":")), a
        return None

    def stops(self, defaults: Optional[Dict] = None) -> Dict:
        """the stop conditions that differ from "none" — the keyword arguments of the engine's admit; {}: the request asks for none"""
        d = defaults or {}
        ids = d.get("stop_token_ids", ()) if self.stop_token_ids is None else self.stop_token_ids
        n = d.get("min_new_tokens", 0) if self.min_new_tokens is None else self.min_new_tokens
        out = {}
        if ids:
            out["stop_token_ids"] = [int(t) for t in ids]
        if self.stop_sequences:
            out["stop_sequences"] = [[int(t) for t in q] for q in self.stop_sequences]
        if n:
            out["min_new_tokens"] = int(n)
        return out

    def sampling(self, defaults: Dict) -> Dict:
        """the request's four sampling settings, `defaults` (a dict of the four) where it sets none of its own"""
        out = {}
        for name in SAMPLING:
            v = getattr(self, name)
            out[name] = defaults[name] if v is None else v
        out["top_k"] = int(out["top_k"] or 0)
        return out

    def controls(self, defaults: Optional[Dict] = None) -> Dict:
        """the controls that differ from "off" — the keyword arguments of the engine's admit; {}: the request asks for none"""
        d = defaults or {}
        out = {}
        for name, off in (("repetition_penalty", 1.0), ("presence_penalty", 0.0), ("frequency_penalty", 0.0)):
            v = getattr(self, name)
            v = d.get(name, off) if v is None else v
            if float(v) != off:
                out[name] = float(v)
        if self.logit_bias:
            out["logit_bias"] = dict(self.logit_bias)
        return out


def _token_ids(v, empty: bool = False) -> bool:
    """a list of token ids: integers >= 0, no booleans (JSON's true is no token 1); `empty`: the list may hold none"""
    return isinstance(v, list) and (empty or bool(v)) and all(isinstance(t, int) and not isinstance(t, bool) and t >= 0 for t in v)


def _json_objects(lines: Sequence[str]):
    """(index, object) of every line that holds a JSON object.  Blank and malformed lines and other JSON values are skipped: the
    checks that run before anything is loaded leave them to parse_requests / parse_prefixes, which name them"""
    for i, line in enumerate(lines):
        try:
            d = json.loads(line) if line.strip() else None
        except json.JSONDecodeError:
            d = None
        if isinstance(d, dict):
            yield i, d


def _number(v) -> bool:
    """a finite number, also as the fp32 value the engine's parameter row holds"""
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and math.isfinite(fp32(v))


def parse_controls(d: dict, where: str) -> Dict:
    """the logit-processor fields of one request object, validated; only those present"""
    out = {}
    if "repetition_penalty" in d:
        if not _number(d["repetition_penalty"]) or fp32(d["repetition_penalty"]) <= 0:
            raise ValueError(f"{where}: \"repetition_penalty\" must be a finite number > 0 (1: off)")
        out["repetition_penalty"] = float(d["repetition_penalty"])
    for name in ("presence_penalty", "frequency_penalty"):
        if name in d:
            if not _number(d[name]):
                raise ValueError(f"{where}: \"{name}\" must be a finite number")
            out[name] = float(d[name])
    if "logit_bias" in d:
        b = d["logit_bias"]
        if not isinstance(b, dict) or not all(isinstance(k, str) and k.isdigit() and _number(v) for k, v in b.items()):
            raise ValueError(f"{where}: \"logit_bias\" must be an object of token ids and finite numbers, {{\"<id>\": value}}")
        out["logit_bias"] = {k: float(v) for k, v in b.items()}
    return out


def parse_sampling(d: dict, where: str) -> Dict:
    """the sampling fields and the seed of one request object, validated; only those present"""
    out = {}
    if "temperature" in d:
        if not _number(d["temperature"]) or d["temperature"] < 0:
            raise ValueError(f"{where}: \"temperature\" must be a finite number >= 0")
        out["temperature"] = float(d["temperature"])
    if "top_k" in d:
        if not isinstance(d["top_k"], int) or isinstance(d["top_k"], bool) or not 0 <= d["top_k"] < 2 ** 31:
            raise ValueError(f"{where}: \"top_k\" must be a non-negative integer (0: off)")
        out["top_k"] = int(d["top_k"])
    if "top_p" in d:
        if not _number(d["top_p"]) or fp32(d["top_p"]) <= 0:
            raise ValueError(f"{where}: \"top_p\" must be a finite number > 0 (1: off)")
        out["top_p"] = float(d["top_p"])
    if "min_p" in d:
        if not _number(d["min_p"]) or d["min_p"] < 0 or fp32(d["min_p"]) >= 1:
            raise ValueError(f"{where}: \"min_p\" must be a number in [0, 1) (0: off)")
        out["min_p"] = float(d["min_p"])
    if "seed" in d:
        if not isinstance(d["seed"], int) or isinstance(d["seed"], bool) or not 0 <= d["seed"] < 2 ** 63:
            raise ValueError(f"{where}: \"seed\" must be a non-negative integer below 2^63")
        out["seed"] = int(d["seed"])
    return out


def parse_sparsity(d: dict, where: str) -> Dict:
    """the "sparsity" field of one request object, validated; {} if absent"""
    if "sparsity" not in d:
        return {}
    v = d["sparsity"]
    if not _number(v) or not 0 <= v < 1:
        raise ValueError(f"{where}: \"sparsity\" must be a number in [0, 1) (0: every row kept)")
    return {"sparsity": float(v)}


def _capped(levels: set) -> List[float]:
    """the distinct levels of one run, ascending; more than MAX_LEVELS are refused"""
    if len(levels) > MAX_LEVELS:
        raise ValueError(f"{len(levels)} distinct \"sparsity\" levels: at most {MAX_LEVELS} in one run (each is resolved to its own "
                         "thresholds before anything runs)")
    return sorted(levels)


def sparsity_levels_of(requests) -> List[float]:
    """the distinct levels the requests carry, ascending; more than MAX_LEVELS are refused"""
    return _capped({float(r.sparsity) for r in requests if r.sparsity is not None})


def check_sparsity_fields(request_lines: Sequence[str], servable=None) -> List[float]:
    """the distinct "sparsity" levels of the request lines, ascending — needs no tokenizer, so it runs before anything is loaded:
    a level outside [0, 1), more than MAX_LEVELS levels and a level `servable(level)` gives a reason against are refused"""
    levels = set()
    for i, d in _json_objects(request_lines):
        lv = parse_sparsity(d, f"request line {i + 1}").get("sparsity")
        if lv is not None:
            why = servable(lv) if servable is not None else None
            if why is not None:
                raise ValueError(f"request line {i + 1}: \"sparsity\" {lv:g}: {why}")
            levels.add(lv)
    return _capped(levels)


def parse_stops(d: dict, where: str, tokenizer=None) -> Dict:
    """the stop-condition fields of one request object, validated; only those present.  "stop": strings, each encoded without a BOS
    into one more stop sequence (needs a tokenizer) — the match stays on token ids: a text the model spells with other tokens than
    the tokenizer gave for the string alone is not caught."""
    out = {}
    if "stop_token_ids" in d:
        v = d["stop_token_ids"]
        if not _token_ids(v, empty=True) or len(set(v)) > MAX_IDS:
            raise ValueError(f"{where}: \"stop_token_ids\" must be a list of at most {MAX_IDS} token ids")
        out["stop_token_ids"] = [int(t) for t in v]
    seqs = []
    if "stop_sequences" in d:
        v = d["stop_sequences"]
        if not isinstance(v, list) or not all(_token_ids(q) and len(q) <= MAX_SEQ_LEN for q in v):
            raise ValueError(f"{where}: \"stop_sequences\" must be a list of lists of 1..{MAX_SEQ_LEN} token ids")
        seqs += [[int(t) for t in q] for q in v]
    if "stop" in d:
        v = d["stop"]
        if not isinstance(v, list) or not all(isinstance(x, str) and x for x in v):
            raise ValueError(f"{where}: \"stop\" must be a list of non-empty strings")
        if tokenizer is None:
            raise ValueError(f"{where}: \"stop\" strings need a tokenizer (a checkpoint), not --synthetic: give \"stop_sequences\" of token ids")
        for x in v:
            q = [int(t) for t in tokenizer.encode(x)]
            if not 1 <= len(q) <= MAX_SEQ_LEN:
                raise ValueError(f"{where}: the \"stop\" string {x!r} encodes to {len(q)} tokens: a stop sequence has 1..{MAX_SEQ_LEN}")
            seqs.append(q)
    if len(seqs) > MAX_SEQS:
        raise ValueError(f"{where}: {len(seqs)} stop sequences (\"stop_sequences\" and \"stop\" together): at most {MAX_SEQS}")
    if seqs or "stop_sequences" in d or "stop" in d:
        out["stop_sequences"] = seqs
    if "min_new_tokens" in d:
        v = d["min_new_tokens"]
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v < 2 ** 31:
            raise ValueError(f"{where}: \"min_new_tokens\" must be a non-negative integer")
        out["min_new_tokens"] = int(v)
    return out


def parse_constraint_fields(d: dict, where: str, tokenizer=None, constraints: Optional[Dict] = None) -> Dict:
    """the constraint fields of one request object, validated; only the one present.  "choices" strings are each encoded alone,
    WITHOUT a BOS (needs a tokenizer) — the match stays on token ids, with the caveat of "stop" strings."""
    kinds = [k for k in ("constraint", "choices", "allowed_token_ids") if k in d]
    if len(kinds) > 1:
        raise ValueError(f"{where}: at most one of \"constraint\", \"choices\" and \"allowed_token_ids\", got " + " and ".join(f'"{k}"' for k in kinds))
    if "constraint" in d:
        c = d["constraint"]
        if not isinstance(c, str) or c not in (constraints or {}):
            raise ValueError(f"{where}: unknown constraint {c!r}" + ("" if constraints else " (no constraints were given)"))
        return {"constraint": c}
    if "choices" in d:
        v = d["choices"]
        if not isinstance(v, list) or not v or not (all(_token_ids(q) for q in v) or all(isinstance(q, str) and q for q in v)):
            raise ValueError(f"{where}: \"choices\" must be a non-empty list of non-empty token id lists, or of non-empty strings")
        if isinstance(v[0], str):
            if tokenizer is None:
                raise ValueError(f"{where}: \"choices\" strings need a tokenizer (a checkpoint), not --synthetic: give lists of token ids")
            enc = []
            for x in v:
                q = [int(t) for t in tokenizer.encode(x)]
                if not q:
                    raise ValueError(f"{where}: the \"choices\" string {x!r} encodes to no tokens")
                enc.append(q)
            v = enc
        return {"choices": [[int(t) for t in q] for q in v]}
    if "allowed_token_ids" in d:
        if not _token_ids(d["allowed_token_ids"]):
            raise ValueError(f"{where}: \"allowed_token_ids\" must be a non-empty list of token ids")
        return {"allowed_token_ids": [int(t) for t in d["allowed_token_ids"]]}
    return {}


FORCED_FIELDS = ("forced_tokens", "forced_text")


def parse_forced(d: dict, where: str, tokenizer=None) -> Dict:
    """the forced-token field of one request object, validated; {} if absent.  "forced_text" is encoded alone, WITHOUT a BOS (needs
    a tokenizer) — the tokens are what the tokenizer gives for the string by itself, with the caveat of "stop" strings: a
    continuation the model would spell with other tokens after this prompt is scored as THESE tokens.  Without a tokenizer
    everything that needs none is still refused (check_forced_fields, before anything is loaded), and {} is returned for a
    well-formed "forced_text"."""
    kinds = [k for k in FORCED_FIELDS if k in d]
    if not kinds:
        return {}
    if len(kinds) > 1:
        raise ValueError(f"{where}: at most one of \"forced_tokens\" and \"forced_text\", got both")
    both = [k for k in ("constraint", "choices", "allowed_token_ids") if k in d]
    if both:
        raise ValueError(f"{where}: \"{kinds[0]}\" does not combine with \"{both[0]}\": a forced token may be one the automaton bans")
    n = d.get("max_new_tokens")
    budget = n if isinstance(n, int) and not isinstance(n, bool) else None
    if "forced_tokens" in d:
        toks = d["forced_tokens"]
        if not _token_ids(toks):
            raise ValueError(f"{where}: \"forced_tokens\" must be a non-empty list of token ids")
    else:
        x = d["forced_text"]
        if not isinstance(x, str) or not x:
            raise ValueError(f"{where}: \"forced_text\" must be a non-empty string")
        if tokenizer is None:
            return {}
        toks = [int(t) for t in tokenizer.encode(x)]
        if not toks:
            raise ValueError(f"{where}: the \"forced_text\" {x!r} encodes to no tokens")
    if budget is not None and budget < len(toks):
        raise ValueError(f"{where}: \"max_new_tokens\" {budget} is below the {len(toks)} forced tokens (leave it out to score them only)")
    return {"forced_tokens": [int(t) for t in toks]}


def check_forced_fields(request_lines: Sequence[str], prefix_lines: Sequence[str] = (), tokenizer_expected: bool = True) -> bool:
    """whether some request line carries forced tokens — needs no tokenizer, so it runs before anything is loaded: an empty list,
    non-integers, both fields on one line, either field next to a constraint field, a budget below the number of forced tokens,
    "forced_text" where no tokenizer will be there (tokenizer_expected False) and either field on a prefix line are refused"""
    for i, d in _json_objects(prefix_lines):
        for k in FORCED_FIELDS:
            if k in d:
                raise ValueError(f"prefix line {i + 1}: \"{k}\" belongs to a request line: a prefix's rows come from the prompt pass, "
                                 "which draws nothing")
    found = False
    for i, d in _json_objects(request_lines):
        parse_forced(d, f"request line {i + 1}")
        if "forced_text" in d and not tokenizer_expected:
            raise ValueError(f"request line {i + 1}: \"forced_text\" needs a tokenizer (a checkpoint), not --synthetic: give "
                             "\"forced_tokens\"")
        found = found or any(k in d for k in FORCED_FIELDS)
    return found


def parse_constraints(lines: Sequence[str]) -> Dict[str, Automaton]:
    """JSON Lines, one token automaton per line: {"id": "yes-no", "states": [{"edges": [[token, next], ...], "default": -1,
    "accept": true}, ...]} (state 0 is the start).  Blank lines are skipped; an empty file is an empty mapping."""
    out: Dict[str, Automaton] = {}
    for i, line in enumerate(lines):
        if not line.strip():
            continue
        try:
            d = json.loads(line)
        except json.JSONDecodeError as e:
            raise ValueError(f"constraint line {i + 1}: not JSON ({e})") from None
        if not isinstance(d, dict) or not isinstance(d.get("id"), str) or not d["id"]:
            raise ValueError(f"constraint line {i + 1}: needs an \"id\" (a non-empty string)")
        if d["id"] in out:
            raise ValueError(f"constraint line {i + 1}: duplicate id {d['id']!r}")
        try:
            out[d["id"]] = Automaton.from_json(d)
        except ValueError as e:
            raise ValueError(f"constraint line {i + 1}: {e}") from None
    return out


def check_constraint_ids(request_lines: Sequence[str], constraints: Dict) -> None:
    """every "constraint" a request line names is an id of `constraints` — needs no tokenizer, so it runs before anything is loaded"""
    for i, d in _json_objects(request_lines):
        if d.get("constraint") is not None and d["constraint"] not in constraints:
            raise ValueError(f"request line {i + 1}: unknown constraint {d['constraint']!r}")


def parse_prefixes(lines: Sequence[str], tokenizer=None) -> Dict[str, List[int]]:
    """JSON Lines, one shared prefix per line: {"id": "sys", "tokens": [...]} or {"id": "sys", "prompt": "..."} (needs a tokenizer;
    BOS prepended as for prompts).  Blank lines are skipped; an empty file is an empty mapping."""
    out: Dict[str, List[int]] = {}
    for i, line in enumerate(lines):
        if not line.strip():
            continue
        try:
            d = json.loads(line)
        except json.JSONDecodeError as e:
            raise ValueError(f"prefix line {i + 1}: not JSON ({e})") from None
        if not isinstance(d, dict) or not isinstance(d.get("id"), str) or not d["id"]:
            raise ValueError(f"prefix line {i + 1}: needs an \"id\" (a non-empty string)")
        if "sparsity" in d:
            raise ValueError(f"prefix line {i + 1}: \"sparsity\" belongs to a request line: a prefix's rows are computed once, by the "
                             "dense prompt pass")
        for k in FORCED_FIELDS:
            if k in d:
                raise ValueError(f"prefix line {i + 1}: \"{k}\" belongs to a request line: a prefix's rows come from the prompt pass, "
                                 "which draws nothing")
        if ("tokens" in d) == ("prompt" in d):
            raise ValueError(f"prefix line {i + 1}: needs exactly one of \"tokens\" and \"prompt\"")
        if d["id"] in out:
            raise ValueError(f"prefix line {i + 1}: duplicate id {d['id']!r}")
        if "tokens" in d:
            toks = d["tokens"]
            if not _token_ids(toks):
                raise ValueError(f"prefix line {i + 1}: \"tokens\" must be a non-empty list of token ids")
        else:
            if tokenizer is None:
                raise ValueError(f"prefix line {i + 1}: a \"prompt\" needs a tokenizer (a checkpoint), not --synthetic")
            if not isinstance(d["prompt"], str):
                raise ValueError(f"prefix line {i + 1}: \"prompt\" must be a string")
            toks = [tokenizer.bos_id()] + tokenizer.encode(d["prompt"])
        out[d["id"]] = [int(t) for t in toks]
    return out


def check_prefix_ids(request_lines: Sequence[str], prefix_lines: Sequence[str]) -> None:
    """every "prefix" a request line names is an "id" of a prefix line — needs no tokenizer, so it runs before anything is loaded"""
    ids = {d.get("id") for _, d in _json_objects(prefix_lines)}
    for i, d in _json_objects(request_lines):
        if d.get("prefix") is not None and d["prefix"] not in ids:
            raise ValueError(f"request line {i + 1}: unknown prefix {d['prefix']!r}" + ("" if ids else " (no prefixes were given)"))


def parse_requests(lines: Sequence[str], default_max_new_tokens: int, tokenizer=None, eos_id: Optional[int] = None,
                   prefixes: Optional[Dict[str, List[int]]] = None, constraints: Optional[Dict[str, Automaton]] = None) -> List[Request]:
    """JSON Lines, one request per line: {"tokens": [...]} or {"prompt": "..."} (needs a tokenizer; BOS prepended as generate.py
    does), with an optional "max_new_tokens" (default: `default_max_new_tokens`).  Blank lines are skipped.  A line may carry
    "prefix": an id of `prefixes`; its tokens / prompt are then the suffix, and a prompt is encoded WITHOUT a BOS (the prefix
    holds it).  A line may carry its own logit processors: "repetition_penalty" (> 0), "presence_penalty", "frequency_penalty"
    and "logit_bias" ({"<id>": value}), its own sampling settings: "temperature" (>= 0), "top_k" (0: off), "top_p" (> 0; 1: off) and
    "min_p" (in [0, 1); 0: off), and its own "seed".  A line may carry its own stop conditions: "stop_token_ids" (at most 16),
    "stop_sequences" (at most 8 lists of 1..8 token ids), "min_new_tokens" and, with a tokenizer, "stop": strings, each encoded
    WITHOUT a BOS into one more stop sequence.  The match is on token ids against the tokens the request generates: a string the
    model spells with other tokens (another split, a leading-space variant) is not caught.  A line may carry ONE constraint:
    "constraint" (an id of `constraints`), "choices" (token id lists, or strings — each encoded alone WITHOUT a BOS, with the same
    caveat; the request produces exactly one of them and then the EOS id, so it needs `eos_id`) or "allowed_token_ids".  A line may
    carry its own "sparsity" (in [0, 1); at most 8 distinct levels in one file).  A line may carry "forced_tokens" (token ids) or,
    with a tokenizer, "forced_text" (encoded alone WITHOUT a BOS, with the caveat of "stop" strings): the request's first draws
    yield these tokens, and the result reports their log-likelihood.  Such a line without "max_new_tokens" gets a budget of their
    number (it only scores them); a larger budget goes on sampling behind them.  Neither combines with a constraint field."""
    out = []
    for i, line in enumerate(lines):
        if not line.strip():
            continue
        try:
            d = json.loads(line)
        except json.JSONDecodeError as e:
            raise ValueError(f"request line {i + 1}: not JSON ({e})") from None
        if not isinstance(d, dict) or ("tokens" in d) == ("prompt" in d):
            raise ValueError(f"request line {i + 1}: needs exactly one of \"tokens\" and \"prompt\"")
        pid = d.get("prefix")
        if pid is not None and (not isinstance(pid, str) or pid not in (prefixes or {})):
            raise ValueError(f"request line {i + 1}: unknown prefix {pid!r}" + ("" if prefixes else " (no prefixes were given)"))
        if "tokens" in d:
            toks = d["tokens"]
            if not _token_ids(toks):
                raise ValueError(f"request line {i + 1}: \"tokens\" must be a non-empty list of token ids")
        else:
            if tokenizer is None:
                raise ValueError(f"request line {i + 1}: a \"prompt\" needs a tokenizer (a checkpoint), not --synthetic")
            toks = ([] if pid is not None else [tokenizer.bos_id()]) + tokenizer.encode(d["prompt"])
            if not toks:
                raise ValueError(f"request line {i + 1}: the \"prompt\" under prefix {pid!r} encodes to no tokens (an empty suffix)")
        if "forced_text" in d and tokenizer is None:
            raise ValueError(f"request line {i + 1}: \"forced_text\" needs a tokenizer (a checkpoint), not --synthetic: give \"forced_tokens\"")
        frc = parse_forced(d, f"request line {i + 1}", tokenizer)
        n = d.get("max_new_tokens", len(frc["forced_tokens"]) if frc else default_max_new_tokens)
        if not isinstance(n, int) or isinstance(n, bool) or n < 1:
            raise ValueError(f"request line {i + 1}: \"max_new_tokens\" must be a positive integer")
        con = parse_constraint_fields(d, f"request line {i + 1}", tokenizer, constraints)
        if "choices" in con and eos_id is None:
            raise ValueError(f"request line {i + 1}: \"choices\" needs an EOS id (--eos_id): a finished choice ends on it, and without "
                             "one its last state is a dead end")
        out.append(Request([int(t) for t in toks], n, eos_id, prefix=pid, **parse_controls(d, f"request line {i + 1}"),
                           **parse_sampling(d, f"request line {i + 1}"), **parse_stops(d, f"request line {i + 1}", tokenizer), **con,
                           **parse_sparsity(d, f"request line {i + 1}"), **frc))
    if not out:
        raise ValueError("no requests")
    sparsity_levels_of(out)
    return out


def _prefix_len(i: int, r: Request, prefixes) -> int:
    """rows of request i's prefix (0: none); `prefixes` maps an id to its tokens"""
    if r.prefix is None:
        return 0
    if not prefixes or r.prefix not in prefixes:
        raise ValueError(f"request {i}: unknown prefix {r.prefix!r}")
    return len(prefixes[r.prefix])


def cache_rows(requests: Sequence[Request], block_size: int, prefixes: Optional[Dict[str, List[int]]] = None) -> int:
    """the cache length a run needs: the longest (prefix +) prompt + budget, capped at block_size; a request that cannot fit is
    refused"""
    rows = []
    for i, r in enumerate(requests):
        P = _prefix_len(i, r, prefixes)
        if P + len(r.tokens) + r.max_new_tokens > block_size:
            raise ValueError(f"request {i}: " + (f"{P} prefix tokens + " if P else "") + f"{len(r.tokens)} prompt tokens + "
                             f"{r.max_new_tokens} new tokens exceed the model's block_size {block_size}")
        rows.append(P + len(r.tokens) + r.max_new_tokens)
    return min(max(rows), block_size)


# ---- the per-request features: one object each ------------------------------------------------------------------------------------
class _Feature:
    """What the batcher asks of a per-request feature; every feature below overrides what it needs and nothing else.

    __init__ takes the batcher's defaults for the feature and validates them with the feature's parser.
    plan(eng, requests), before anything runs: refuses what must be refused, switches the engine feature on if the run wants it —
    once per batcher (`on`): the switch drops the engine's captured step, and a later run() keeps it — registers what the engine
    must hold, and keeps per request the keywords its admission gets (`kw`; "temperature" and "top_k" are the admission's two
    positionals).  Then, per sync point, sync(eng, state, slot_req); per finished request r in slot s with n tokens,
    harvest(eng, s, r, n); and result(eng): the keys the feature adds to the result."""

    on = False   # switched on at the engine
    kw = ()      # per request of the planned run: its admission's keywords (empty: none for any request)

    def switch_on(self, set_feature, *args):
        if not self.on:
            set_feature(*args)
            self.on = True

    def admit_kw(self, r: int) -> Dict:
        return self.kw[r] if self.kw else {}

    def sync(self, eng, state, slot_req):
        pass

    def harvest(self, eng, s: int, r: int, n: int):
        pass

    def result(self, eng) -> Dict:
        return {}


class Prefixes(_Feature):
    """Shared prefixes: a request may name a prefix — a token sequence registered with the engine once, whose K / V rows stay in a
    device store.  Its own tokens are then the suffix: it is served as prompt = prefix + suffix, but its admission copies the
    prefix's rows into the slot and runs the prompt pass over the suffix alone.  Prefixes are named, never detected: what a request
    computes does not depend on what happened to be cached when it was admitted.
    `prefixes` (id -> tokens): the engine also offers has_prefix(id), register_prefix(id, tokens) and admit(..., prefix=id); every
    prefix the engine does not hold yet is registered before the first admission (the engine is idle), named by a request or not,
    and only requests that name one are admitted with `prefix=`."""

    def __init__(self, prefixes):
        self.prefixes = {k: [int(t) for t in v] for k, v in (prefixes or {}).items()}

    def plan(self, eng, requests):
        for name, toks in self.prefixes.items():
            if not eng.has_prefix(name):
                eng.register_prefix(name, toks)
        self.rows = [_prefix_len(i, r, self.prefixes) for i, r in enumerate(requests)]
        self.kw = [{"prefix": r.prefix} if P else {} for r, P in zip(requests, self.rows)]

    def result(self, eng):  # (every request was admitted once)
        return {"prefix_admissions": sum(1 for P in self.rows if P), "prefix_rows_reused": sum(self.rows),
                "prefix_paths": dict(getattr(eng, "prefix_paths", {}))}


class Logprobs(_Feature):
    """`logprobs` (None: off; 0: each token's logprob under the model's own distribution — temperature 1, no top-k filter; 1..8:
    and that many most likely alternates): the engine also offers set_logprobs(n) and read_logprobs(slot, n) -> (lp, top_ids,
    top_lp) lists aligned with read_history(slot, n); the result gains "logprobs" and, for n > 0, "top_logprobs"."""

    def __init__(self, logprobs):
        if logprobs is not None and (isinstance(logprobs, bool) or not isinstance(logprobs, int) or not 0 <= logprobs <= 8):
            raise ValueError("logprobs must be None or an integer in 0..8")
        self.n = logprobs

    def plan(self, eng, requests):
        if self.n is not None:
            self.switch_on(eng.set_logprobs, self.n)
        self.lps: List[Optional[List[float]]] = [None] * len(requests)
        self.tops: List[Optional[List]] = [None] * len(requests)

    def harvest(self, eng, s, r, n):
        if self.on:
            lp, ids, tlp = eng.read_logprobs(s, n)
            self.lps[r] = [float(v) for v in lp]
            self.tops[r] = [[(int(i), float(v)) for i, v in zip(ii, vv)] for ii, vv in zip(ids, tlp)]

    def result(self, eng):
        if not self.on:
            return {}
        return {"logprobs": self.lps, **({"top_logprobs": self.tops} if self.n > 0 else {})}


class Processors(_Feature):
    """Logit processors: `repetition_penalty`, `presence_penalty` and `frequency_penalty` are the defaults of requests that set
    none of their own (Request.controls).  When any request (or a default) asks for a processor the engine also offers
    set_logit_processors(True) and admit(..., repetition_penalty=, presence_penalty=, frequency_penalty=, logit_bias=); only
    requests that ask for one are admitted with those keywords."""

    def __init__(self, repetition_penalty, presence_penalty, frequency_penalty):
        self.defaults = parse_controls({"repetition_penalty": repetition_penalty, "presence_penalty": presence_penalty,
                                        "frequency_penalty": frequency_penalty}, "ContinuousBatcher")

    def plan(self, eng, requests):
        self.kw = [r.controls(self.defaults) for r in requests]
        if any(self.kw):
            self.switch_on(eng.set_logit_processors, True)


class Sampling(_Feature):
    """Sampling: `temperature`, `top_k`, `top_p` and `min_p` are the defaults of requests that set none of their own
    (Request.sampling).  When a default or some request differs from (temperature, top_k, 1, 0) — what the fused top-k samplers
    serve from the batcher's two scalars — the engine also offers set_sampling_params(True) and admit(..., top_p=, min_p=); every
    request is then admitted with its own four settings, in this run and in every later one, which hold for all of its draws, and
    run_steps' temperature and top_k no longer matter."""

    def __init__(self, temperature, top_k, top_p, min_p):
        parse_sampling({"top_p": top_p, "min_p": min_p}, "ContinuousBatcher")
        self.temperature = temperature
        self.base = {"temperature": temperature, "top_k": int(top_k or 0), "top_p": float(top_p), "min_p": float(min_p)}

    def plan(self, eng, requests):
        sampling = [r.sampling(self.base) for r in requests]
        plain = dict(self.base, top_p=1.0, min_p=0.0)
        if any(s != plain for s in sampling):
            self.switch_on(eng.set_sampling_params, True)
        self.kw = sampling if self.on else ()


class Stops(_Feature):
    """Stop conditions: a request may carry stop token ids, stop sequences of token ids and a minimum length (stopping.py).  They
    are matched on the device inside the step, so a request ends on the very step its stop appears whatever sync_every is.
    `stop_token_ids` and `min_new_tokens` are the defaults of requests that set none of their own (Request.stops).  When a default
    or some request asks for a stop id, a stop sequence or a minimum, or `finish_reason` is set, the engine also offers
    set_stop_conditions(True), admit(..., stop_token_ids=, stop_sequences=, min_new_tokens=) — only requests that ask for one are
    admitted with those keywords — and read_finish(slot) -> (reason, match); the result gains "finish_reason" ("stop_token" /
    "stop_sequence" / "length" / "cache" per request, in input order) and "stop_match" (the token id, the sequence's index, or -1).
    "tokens" stays every token drawn, the stopping ones included."""

    def __init__(self, stop_token_ids, min_new_tokens, finish_reason):
        self.defaults = parse_stops({"stop_token_ids": list(stop_token_ids or ()), "min_new_tokens": min_new_tokens}, "ContinuousBatcher")
        self.finish_reason = bool(finish_reason)

    def plan(self, eng, requests):
        self.kw = [r.stops(self.defaults) for r in requests]
        if self.finish_reason or any(self.kw):
            self.switch_on(eng.set_stop_conditions, True)
        self.reasons: List[Optional[str]] = [None] * len(requests)
        self.matches: List[int] = [-1] * len(requests)

    def harvest(self, eng, s, r, n):
        if self.on:
            self.reasons[r], self.matches[r] = eng.read_finish(s)

    def result(self, eng):
        return {"finish_reason": self.reasons, "stop_match": self.matches} if self.on else {}


class Constraints(_Feature):
    """Constraints: a request may follow a token automaton (constraints.py) — a registered one by name, one of a list of `choices`,
    or any sequence over `allowed_token_ids` (Request.constraint_spec).  The automaton advances on the device inside the step, so
    every token is drawn under it whatever sync_every is; the match is on token ids, not text.
    `constraints` (id -> Automaton) are what requests may name.  Exactly when some request carries one of the three the engine also
    offers set_constraints(True), has_constraint(id), register_constraint(id, automaton) — one per distinct content — and
    admit(..., constraint=id); only those requests are admitted with the keyword.  `sampling`: the batcher's Sampling, which knows
    the temperature a request is admitted at."""

    def __init__(self, constraints, sampling: Sampling):
        self.constraints, self.sampling = dict(constraints or {}), sampling

    def plan(self, eng, requests):
        self.kw = [{} for _ in requests]
        automata: Dict[str, Automaton] = {}
        for i, r in enumerate(requests):
            spec = r.constraint_spec()
            if spec is None:
                continue
            name, a = spec
            if a is None:
                if name not in self.constraints:
                    raise ValueError(f"request {i}: unknown constraint {name!r}")
                a = self.constraints[name]
            if r.choices is not None and r.eos_id is None:
                raise ValueError(f"request {i}: choices need an EOS id: a finished choice ends on it")
            try:
                a.check(eng.cfg.vocab_size, r.eos_id)
            except ValueError as e:
                raise ValueError(f"request {i}: {e}") from None
            T = self.sampling.admit_kw(i).get("temperature", self.sampling.temperature)  # what request i is admitted at
            if float(T) > MAX_TEMPERATURE:
                raise ValueError(f"request {i}: a constrained request needs temperature <= {MAX_TEMPERATURE:g}, got {T}")
            self.kw[i]["constraint"], automata[name] = name, a
        if automata:
            self.switch_on(eng.set_constraints, True)
            for name, a in automata.items():
                if not eng.has_constraint(name):
                    eng.register_constraint(name, a)


class Sparsity(_Feature):
    """Per-request sparsity: a request may carry its own sparsity level.  The engine then keeps one threshold per slot on the device
    and an admission writes the slot's column, so one captured step serves any mix of levels.  A step reads the union of the rows
    its active slots keep, each under its own thresholds: a low-sparsity request widens what the whole batch reads.
    `sparsity` is the level the engine was built at (None: unknown) and `sparsity_levels` maps each level a request may carry to
    its per-layer thresholds.  Exactly when some request's level differs from `sparsity` the engine also offers
    set_slot_sparsity(True), admit(..., thresholds=) — only requests at another level than the run's are admitted with the keyword
    — and kept_by_slot(); the result gains "kept_by_request": per request the mean over the sync points it ran up to, and over the
    projections, of the fraction of rows it kept (None: it ran no step that a sync point saw)."""

    def __init__(self, sparsity, sparsity_levels):
        self.sparsity = None if sparsity is None else parse_sparsity({"sparsity": sparsity}, "ContinuousBatcher")["sparsity"]
        self.levels = {float(k): v for k, v in (sparsity_levels or {}).items()}

    def plan(self, eng, requests):
        self.kw = [{} for _ in requests]
        for i, r in enumerate(requests):
            if r.sparsity is None or (self.sparsity is not None and float(r.sparsity) == self.sparsity):
                continue  # the run's own level
            if float(r.sparsity) not in self.levels:
                raise ValueError(f"request {i}: no thresholds for sparsity {float(r.sparsity):g} (sparsity_levels)")
            self.kw[i]["thresholds"] = self.levels[float(r.sparsity)]
        sparsity_levels_of(requests)
        if any(self.kw):
            self.switch_on(eng.set_slot_sparsity, True)
        self.kept_sum, self.kept_n = [0.0] * len(requests), [0] * len(requests)

    def sync(self, eng, state, slot_req):
        if not self.on:
            return
        kept = eng.kept_by_slot()  # of the burst's last step: the slots that ran it (still active, or stopped by it)
        for s, r in enumerate(slot_req):
            ran = (state[SLOT_ACTIVE] >> s) & 1 or (state[SLOT_FINISH + s] == state[SLOT_STEP] - 1 and state[SLOT_PRODUCED + s] >= 2)
            if r is not None and ran:
                self.kept_sum[r] += sum(v[s] for v in kept.values()) / len(kept)
                self.kept_n[r] += 1

    def result(self, eng):
        return {"kept_by_request": [t / n if n else None for t, n in zip(self.kept_sum, self.kept_n)]} if self.on else {}


class Forced(_Feature):
    """Teacher forcing: a request may carry tokens its first draws yield in place of what its sampler drew (forcing.py).  The
    swap happens on the device inside the step, behind the samplers and in front of the logprob and retire launches, so the
    logprob filed under a forced draw is the model's log p(that token | everything before it) and the request ends on a forced EOS
    or stop like on a drawn one, whatever sync_every is.
    Exactly when some request carries forced tokens the engine also offers set_forced_tokens(True) and admit(..., forced_tokens=);
    only those requests are admitted with the keyword.  `logprobs`: the batcher's Logprobs, whose level is raised to at least 1
    when this feature switches on (the top-1 alternate decides "is_greedy"), so the result then holds "logprobs" and "top_logprobs"
    as well.  The result gains, per request in input order (None for a request without forced tokens): "forced" — how many forced
    draws it made, below the number given if an EOS id, a stop condition or the cache ended it first —, "loglikelihood" — the sum
    of those draws' fp32 logprobs, added in draw order in Python floats — and "is_greedy" — whether every one of those tokens was
    its row's top-1 id."""

    def __init__(self, logprobs: Logprobs):
        self.logprobs = logprobs

    def plan(self, eng, requests):
        self.given = [list(r.forced_tokens) if r.forced_tokens else None for r in requests]
        self.kw = [{"forced_tokens": g} if g else {} for g in self.given]
        for i, (r, g) in enumerate(zip(requests, self.given)):
            if g and len(g) > r.max_new_tokens:
                raise ValueError(f"request {i}: {len(g)} forced tokens exceed its budget of {r.max_new_tokens}")
            if g and r.constraint_spec() is not None:
                raise ValueError(f"request {i}: forced tokens do not combine with a constraint")
            if g and not all(0 <= t < eng.cfg.vocab_size for t in g):
                raise ValueError(f"request {i}: a forced token id is outside the vocabulary 0..{eng.cfg.vocab_size - 1}")
        if any(self.kw):
            lp = self.logprobs
            if not lp.on or lp.n < 1:  # the level the verdicts below need
                lp.n, lp.on = max(1, lp.n or 0), False
                lp.switch_on(eng.set_logprobs, lp.n)
            self.switch_on(eng.set_forced_tokens, True)
        self.counts: List[Optional[int]] = [None] * len(requests)
        self.sums: List[Optional[float]] = [None] * len(requests)
        self.greedy: List[Optional[bool]] = [None] * len(requests)

    def harvest(self, eng, s, r, n):
        g = self.given[r]
        if not self.on or not g:
            return
        k = min(len(g), n)  # draws 0 .. k-1 were forced: the request's first k tokens ARE g[:k]
        lps, tops = self.logprobs.lps[r], self.logprobs.tops[r]
        total = 0.0
        for v in lps[:k]:
            total += float(v)
        self.counts[r], self.sums[r] = k, total
        self.greedy[r] = all(tops[i][0][0] == g[i] for i in range(k))

    def result(self, eng):
        return {"forced": self.counts, "loglikelihood": self.sums, "is_greedy": self.greedy} if self.on else {}


class ContinuousBatcher:
    """Runs requests through an engine with B slots.  The engine offers B, max_seq, admit(slot, tokens, budget, eos_id, seed,
    temperature, top_k), run_steps(k, temperature, top_k, use_graph), read_state() (the slot state words, one copy),
    read_history(slot, n) and union_kept().  Every other keyword belongs to one of `features` — Prefixes, Logprobs, Processors,
    Sampling, Stops, Constraints, Sparsity and Forced above, which say what they add to this protocol: while none is asked for, an engine
    needs none of their methods and every call is the one above.  run() may be called again: what a feature switched on stays on."""

    def __init__(self, engine, sync_every: int = 8, refill: str = "free", temperature: float = 0.8, top_k: Optional[int] = 200,
                 seed: int = 1234, use_graph: bool = True, prefixes: Optional[Dict[str, List[int]]] = None,
                 logprobs: Optional[int] = None, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                 frequency_penalty: float = 0.0, top_p: float = 1.0, min_p: float = 0.0, stop_token_ids=(), min_new_tokens: int = 0,
                 finish_reason: bool = False, constraints: Optional[Dict[str, Automaton]] = None, sparsity: Optional[float] = None,
                 sparsity_levels: Optional[Dict[float, List[Dict[str, float]]]] = None):
        if refill not in REFILL:
            raise ValueError(f"refill must be one of {REFILL}")
        if int(sync_every) < 1:
            raise ValueError("sync_every must be >= 1")
        self.eng, self.K, self.refill = engine, int(sync_every), refill
        self.temperature, self.top_k, self.seed, self.use_graph = temperature, top_k, int(seed), use_graph
        sampling = Sampling(temperature, top_k, top_p, min_p)
        lps = Logprobs(logprobs)
        self.features = [Prefixes(prefixes), lps, Processors(repetition_penalty, presence_penalty, frequency_penalty),
                         sampling, Stops(stop_token_ids, min_new_tokens, finish_reason), Constraints(constraints, sampling),
                         Sparsity(sparsity, sparsity_levels), Forced(lps)]
        self.prefixes = self.features[0].prefixes  # (the fit check counts a prefix's rows)

    def _clock(self):
        try:
            import torch
            if torch.cuda.is_available():
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                return e
        except ImportError:
            pass
        return time.perf_counter()

    @staticmethod
    def _seconds(a, b) -> float:
        return (b - a) if isinstance(a, float) else a.elapsed_time(b) / 1000.0

    def run(self, requests: Sequence[Request]) -> Dict:
        eng, B = self.eng, self.eng.B
        for i, r in enumerate(requests):  # refused before anything runs
            P = _prefix_len(i, r, self.prefixes)
            if len(r.tokens) < 1 or r.max_new_tokens < 1 or P + len(r.tokens) + r.max_new_tokens > eng.max_seq:
                raise ValueError(f"request {i}: " + (f"{P} prefix tokens + " if P else "") + f"{len(r.tokens)} prompt tokens + "
                                 f"{r.max_new_tokens} new tokens do not fit a cache of {eng.max_seq} rows")
        for f in self.features:
            f.plan(eng, requests)
        pending = deque(range(len(requests)))
        slot_req: List[Optional[int]] = [None] * B
        admitted_at = [0] * B
        out: List[Optional[List[int]]] = [None] * len(requests)
        slots_used: List[int] = [-1] * len(requests)
        steps = admissions = slot_steps = 0
        step0 = eng.read_state()[SLOT_STEP]  # the engine's step counter (finish steps are on its scale)
        admit_spans = []
        t0 = time.perf_counter()
        c0 = self._clock()
        while pending or any(r is not None for r in slot_req):
            free = [s for s in range(B) if slot_req[s] is None]
            if pending and free and (self.refill == "free" or len(free) == B):
                a0 = self._clock()
                for s in free:
                    if not pending:
                        break
                    r = pending.popleft()
                    q = requests[r]
                    kw = {"temperature": self.temperature, "top_k": self.top_k}
                    for f in self.features:
                        kw.update(f.admit_kw(r))
                    eng.admit(s, q.tokens, q.max_new_tokens, q.eos_id, self.seed + r if q.seed is None else q.seed,
                              kw.pop("temperature"), kw.pop("top_k"), **kw)
                    slot_req[s], admitted_at[s], slots_used[r] = r, step0 + steps, s
                    admissions += 1
                admit_spans.append((a0, self._clock()))
            eng.run_steps(self.K, self.temperature, self.top_k, self.use_graph)
            steps += self.K
            state = eng.read_state()
            for f in self.features:
                f.sync(eng, state, slot_req)
            for s in range(B):
                r = slot_req[s]
                if r is None or (state[SLOT_ACTIVE] >> s) & 1:
                    continue
                out[r] = eng.read_history(s, state[SLOT_PRODUCED + s])
                for f in self.features:
                    f.harvest(eng, s, r, state[SLOT_PRODUCED + s])
                slot_steps += state[SLOT_FINISH + s] - admitted_at[s]
                slot_req[s] = None
        c1 = self._clock()
        if not isinstance(c1, float):
            c1.synchronize()
        wall = time.perf_counter() - t0
        wall_dev = self._seconds(c0, c1)
        t_admit = sum(self._seconds(a, b) for a, b in admit_spans)
        useful = sum(len(o) for o in out)
        res = {
            "tokens": out, "slots": slots_used, "steps": steps, "admissions": admissions, "wall_s": wall,
            "admission_s": t_admit, "admission_share": t_admit / wall_dev if wall_dev > 0 else 0.0,
            "mean_active_slots": slot_steps / steps if steps else 0.0, "useful_tokens": useful,
            "useful_tokens_per_sec": useful / wall if wall > 0 else 0.0, "union_kept": eng.union_kept(),
            "refill": self.refill, "sync_every": self.K, "batch_size": B,
        }
        for f in self.features:
            res.update(f.result(eng))
        return res

