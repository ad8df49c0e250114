"""The deferred-join tail of a launch plan without a GPU: which forward ops are unconsumed (`planExecutor.unconsumed_ops`,
a rule over the dataflow), the order the tail form of a list emits them in, the ticket table of csrc/plan_tail.h under the
host sanitizers in a stand-alone program, and the C ABI's refusals."""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _pe():
    from sparseconvnet import planExecutor
    return planExecutor


# hand-made op lists of the template's own record types, the fields the dataflow rules do not read left empty; buffer 0 =
# the input
def _op(record, *head):
    return record._make(head + (None,) * (len(record._fields) - len(head)))


def _conv(x, y):
    return _op(_pe().Conv, "conv", x, y)


def _bn(x, y):
    return _op(_pe().Bn, "bn", x, y)


def _add(a, b, y):
    return _op(_pe().Add, "add", a, b, y)


# the test's own statement of what an op writes and reads, by tuple position: independent of the records' `.out` / `.ins`
out_of = lambda op: op[3] if op[0] == "add" else op[2]
ins_of = lambda op: (op[1], op[2]) if op[0] == "add" else (op[1],)


def _reaches_an_output(ops, op, outs):
    """the definition, by brute force: an op is consumed when some returned buffer is reachable from what it writes"""
    reach, grew = {out_of(op)}, True
    while grew:
        grew = False
        for o in ops:
            if out_of(o) not in reach and reach & set(ins_of(o)):
                reach.add(out_of(o))
                grew = True
    return bool(reach & set(outs))


CASES = {
    # name: (ops, returned buffers, indices expected unconsumed)
    "chain": ([_conv(0, 1), _bn(1, 2), _conv(2, 3), _bn(3, 4), _conv(4, 5)], [3], {3, 4}),
    "diamond, one arm unconsumed": ([_conv(0, 1), _conv(1, 2), _conv(1, 3), _bn(3, 4), _bn(2, 5)], [5], {2, 3}),
    "a producer read by a consumed and an unconsumed op stays": (
        [_conv(0, 1), _bn(1, 2), _conv(1, 3), _add(3, 2, 4)], [2], {2, 3}),
    "nothing unconsumed": ([_conv(0, 1), _bn(1, 2), _add(1, 2, 3)], [3], set()),
    "everything consumed by a late output": ([_conv(0, 1), _bn(1, 2), _conv(2, 3), _bn(3, 4), _conv(4, 5)], [1, 5], set()),
    "an unconsumed add arm": ([_conv(0, 1), _conv(0, 2), _add(1, 2, 3), _conv(1, 4)], [4], {1, 2}),
    "no output at all": ([_conv(0, 1), _bn(1, 2)], [], {0, 1}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_unconsumed_ops_on_hand_made_lists(name):
    ops, outs, want = CASES[name]
    got = _pe().unconsumed_ops(ops, [(b, None) for b in outs])
    assert set(got) == want
    for i, op in enumerate(ops):
        assert (i in got) == (not _reaches_an_output(ops, op, outs)), (name, i)


def test_tail_emission_is_a_stable_partition_that_keeps_fused_pairs_adjacent():
    pe = _pe()
    # a top-down path: lateral conv + up conv fused with the add (conv -> add), merged conv + the BatchNorm of the next
    # stage (conv -> bn statistics); stage 1 (ops 0-4) is returned, stage 2 (ops 5-9) is not, op 10 is a consumed projection
    ops = [_conv(0, 1), _bn(1, 2), _conv(2, 3), _add(3, 1, 4), _conv(4, 5),
           _bn(5, 6), _conv(6, 7), _conv(0, 8), _add(7, 8, 9), _conv(9, 10),
           _conv(5, 11)]
    outs = [(5, None), (11, None)]
    dead = pe.unconsumed_ops(ops, outs)
    assert set(dead) == {5, 6, 7, 8, 9}
    emit = pe.tail_emission(ops, dead)
    assert sorted(id(o) for o, _ in emit) == sorted(id(o) for o in ops)           # every record, once
    main = [o for o, f in emit if not f & pe.F_TAIL]
    tail = [o for o, f in emit if f & pe.F_TAIL]
    assert emit == [(o, 0) for o in main] + [(o, pe.F_TAIL) for o in tail]         # consumed first, projection included
    assert main == [ops[i] for i in (0, 1, 2, 3, 4, 10)] and tail == [ops[i] for i in (5, 6, 7, 8, 9)]
    # fused pairs: (convolution, the add in its write-out), (convolution, the BatchNorm taking its statistics) stand next
    # to each other on their stream whenever both are in the same class
    for a, b in ((2, 3), (7, 8), (0, 1)):
        lst = tail if a in dead else main
        assert (a in dead) == (b in dead)
        assert lst.index(ops[b]) - lst.index(ops[a]) == 1
    # the one pair that crosses: consumed convolution 4 -> unconsumed BatchNorm 5 (first on the tail)
    assert 4 not in dead and 5 in dead and tail[0] is ops[5]
    # nothing unconsumed: the list as it was
    assert pe.tail_emission(ops[:5], frozenset()) == [(o, 0) for o in ops[:5]]


def test_record_constants_match_the_header():
    import re
    pe = _pe()
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "aabr_hip.h")).read()
    val = lambda n: int(re.search(r"#define %s (\d+)" % n, hdr).group(1))
    assert val("AABR_PLAN_TAIL") == pe.F_TAIL and val("AABR_PLAN_TAIL_JOIN") == pe.K_TAIL_JOIN
    flags = [val(n) for n in ("AABR_PLAN_BF16", "AABR_PLAN_TO_BF16", "AABR_PLAN_SIDE", "AABR_PLAN_JOIN", "AABR_PLAN_TAIL")]
    assert len(set(flags)) == 5 and all(f & (f - 1) == 0 for f in flags)
    assert pe.plan_tail in (0, 1, 2) and pe.PLAN_TAIL_DEFAULT in (0, 1, 2)
    # every record kind and flag of the header, by name, in the record module (and through planExecutor's re-export)
    from sparseconvnet import plan_records
    names = {"CONV": "K_CONV", "CONV_WIDE": "K_WIDE", "CONV_DW": "K_DW", "BN_FWD": "K_BNF", "BN_BWD": "K_BNB", "ADD": "K_ADD",
             "CAST": "K_CAST", "CONV_WIDE_SPLIT": "K_WSPLIT", "CONV_NARROW": "K_NARROW", "CONV_SINGLE": "K_SINGLE",
             "TAIL_JOIN": "K_TAIL_JOIN", "BF16": "F_BF16", "TO_BF16": "F_TO_BF16", "SIDE": "F_SIDE", "JOIN": "F_JOIN",
             "TAIL": "F_TAIL"}
    defined = dict(re.findall(r"#define AABR_PLAN_(\w+) (\d+)", hdr))
    assert sorted(defined) == sorted(names)
    for n, v in defined.items():
        assert getattr(plan_records, names[n]) == getattr(pe, names[n]) == int(v), n
    kinds = [int(v) for n, v in defined.items() if names[n].startswith("K_")]
    assert sorted(kinds) == sorted(plan_records.LAYOUT) and plan_records.SIZE == 176


def test_c_abi_refusals_and_no_op_tickets_without_a_device():
    """what needs no launch: tickets 0 / never handed out / garbage are no-ops for join, sync and release; the one-call
    and the launcher-thread entry refuse tail records; the knob is known"""
    import _hip
    lib = _hip.load()
    for tk in (0, 7, (1 << 20) | 1, (1 << 64) - 1):
        assert lib.aabr_plan_tail_join(tk, None) == 0
        assert lib.aabr_plan_tail_sync(tk) == 0
        assert lib.aabr_plan_tail_release(tk) == 0 and lib.aabr_plan_tail_release(tk) == 0
    assert lib.aabr_set_knob(b"PLAN_TAIL", 1, 0) == 0
    try:
        rec = bytearray(176)
        import struct
        struct.pack_into("<ii", rec, 0, 6, 16)                 # an empty AABR_PLAN_ADD flagged AABR_PLAN_TAIL
        assert lib.aabr_plan_run(bytes(rec), 1, None) == -1
        assert b"aabr_plan_run_tail" in lib.aabr_last_error()
        assert lib.aabr_plan_submit(bytes(rec), 1, None, 0) == -1
        assert b"AABR_PLAN_TAIL" in lib.aabr_last_error()
        assert lib.aabr_plan_run_tail(bytes(rec), 1, None, None) == -1
    finally:
        assert lib.aabr_set_knob(b"PLAN_TAIL", 0, 1) == 0


def test_ticket_table_under_host_sanitizers(tmp_path):
    cxx = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cxx):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "plan_tail_host")
    base = [cxx, "-x", "c++", "-O1", "-g", "-std=c++17", "-pthread", "-o", exe,
            os.path.join(HERE, "plan_tail_host_harness.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0:
        subprocess.check_call(base)                # the program itself must compile; only the runtime may be missing
        pytest.skip("host sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout + r.stderr


def test_a_list_without_side_or_tail_records_needs_no_device():
    """whatever PLAN_TAIL says (the shipped default included), the library looks its streams up at the first record
    that needs one: a plain list is dispatched, and refused or accepted, on a machine without a GPU"""
    import struct
    import _hip
    lib = _hip.load()
    rec = bytearray(176)
    struct.pack_into("<ii", rec, 0, 6, 0)                      # AABR_PLAN_ADD over 0 elements: accepted, no launch
    ticket = ctypes.c_uint64(7)
    for mode in (None, 0, 1, 2):
        assert lib.aabr_set_knob(b"PLAN_TAIL", mode or 0, 1 if mode is None else 0) == 0
        try:
            assert lib.aabr_plan_run(bytes(rec), 1, None) == 0, (mode, lib.aabr_last_error())
            assert lib.aabr_plan_run_tail(bytes(rec), 1, None, ctypes.byref(ticket)) == 0 and ticket.value == 0
        finally:
            assert lib.aabr_set_knob(b"PLAN_TAIL", 0, 1) == 0


_templates = {}


def _small_template(bf16):
    """(network, its real `_Template`) for the small network of tests/test_ref_net_cpu.py in training mode, built without a
    device: the template only asks the plan object for `weights` and `packs`"""
    if bf16 not in _templates:
        import torch
        import sparseconvnet as scn
        from sparseconvnet import SCN
        torch.manual_seed(3)
        dt = torch.bfloat16 if bf16 else torch.float32
        net = scn.FPN_Net([64, 64, 16], 3, ["xyz", "color", "normal"], 1, [8, 8, 16], 8, True, [2, 1], [2, 1],
                          [[[2, 2, 2]] * 2, [[2, 2, 2]] * 2], [[64, 64, 16], [32, 32, 8]], [0, 1, 2, 3], leakiness=0,
                          voxel_scale=4, bn_momentum=0.95, feature_dtype=dt)
        net.train(True)
        plan = type("Plan", (), {})()
        plan.weights = [m.weight for m in net.modules()
                        if isinstance(m, (scn.SubmanifoldConvolution, scn.Convolution, scn.Deconvolution))]
        plan.packs = [(torch.empty(1), torch.empty(1)) for _ in plan.weights]
        tpl = _pe()._Template(net, SCN._key(net.layers_in[0].spatial_size), net.layers_in[1].nOut, dt, plan)
        _templates[bf16] = (net, plan, tpl)
    return _templates[bf16][0], _templates[bf16][2]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_the_real_template_by_field_name(bf16):
    """what the device runs imply about a template, asserted on the CPU through the records' field names"""
    pe = _pe()
    net, t = _small_template(bf16)
    fops, outs = t.fops, [b for b, _ in t.outs]
    kinds = {"add": pe.Add, "cast": pe.Cast, "bn": pe.Bn, "conv": pe.Conv}
    assert all(type(op) is kinds[op.kind] for op in fops)
    assert len(fops) == (39 if bf16 else 32) and {"add", "bn", "conv"} <= {op.kind for op in fops}
    # every buffer but the graph input has exactly one producer; `.out` / `.ins` say what the positions say
    assert sorted(op.out for op in fops) == list(range(1, len(t.fbufs)))
    assert all(op.out == out_of(op) and tuple(op.ins) == ins_of(op) for op in fops)
    # unconsumed ops: the brute-force definition on the real list, for the returned maps and for the first one alone
    assert t.dead == pe.unconsumed_ops(fops, t.outs)
    for some in (outs, outs[:1]):
        got = pe.unconsumed_ops(fops, [(b, None) for b in some])
        assert set(got) == {i for i, op in enumerate(fops) if not _reaches_an_output(fops, op, some)}
    assert pe.unconsumed_ops(fops, [(outs[0], None)])        # (the second case is not an empty one)
    # every fused add rides on a convolution whose only reader it is
    at = {id(op): i for i, op in enumerate(fops)}
    assert len(t.fuse) == 5
    for conv_id, (add, other) in t.fuse.items():
        conv = fops[at[conv_id]]
        assert conv.kind == "conv" and add.kind == "add" and sorted(add.ins) == sorted((conv.out, other))
        assert [op for op in fops if conv.out in op.ins] == [add] and conv.out not in outs
        assert at[id(add)] > at[conv_id] and (other == 0 or other in [op.out for op in fops[:at[conv_id]]])
    # every statistics claim: a convolution directly followed, its fused add aside, by a training BatchNorm that reads
    # what the launch wrote, with the same plane count
    assert len(t.stat_claims) == 8
    for conv_id in t.stat_claims:
        i = at[conv_id]
        conv, wrote, nxt = fops[i], [fops[i].out], fops[i + 1]
        if conv_id in t.fuse:
            assert nxt is t.fuse[conv_id][0]
            wrote, nxt = wrote + [nxt.out], fops[i + 2]
        assert conv.kind == "conv" and nxt.kind == "bn" and nxt.train == 1 and nxt.x in wrote and nxt.planes == conv.n_out
    assert not t.cross or set(t.cross.values()) <= t.stat_claims
    # the all-gradients backward list: one slot per trainable parameter, a spare buffer wherever a sum may ride
    assert t.params and all(p.requires_grad for p in t.params)
    bw = t.backward(tuple(True for _ in outs), True)
    bkinds = {"add": pe.Add, "cast": pe.Cast, "bn": pe.BnBwd, "din": pe.Din, "dw": pe.Dw}
    assert all(type(op) is bkinds[op.kind] for op in bw["ops"])
    slots = [op.slot for op in bw["ops"] if op.kind == "dw"]
    slots += [s for op in bw["ops"] if op.kind == "bn" for s in (op.d_weight_slot, op.d_bias_slot) if s >= 0]
    assert len(slots) == len(set(slots)) == len(t.params) and sorted(bw["poff"]) == list(range(len(t.params)))
    assert sorted(slots) == sorted(4 * o for o in bw["poff"].values())
    ends = sorted((o, o + t.params[i].numel()) for i, o in bw["poff"].items())
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] <= bw["ptotal"]
    dins = [op for op in bw["ops"] if op.kind == "din"]
    assert len(dins) == 17 and any(op.res is not None for op in dins)
    assert all((op.res is None) == (op.tmp is None) for op in dins)
    assert all(op.tmp[0] == pe.G and op.tmp != op.gx for op in dins if op.tmp is not None)


def test_no_numeric_subscript_of_an_op_in_the_executor():
    """template ops are read by whole-op unpacking or by field name, never by position"""
    import re
    src = open(os.path.join(os.path.dirname(HERE), "automatic-as-built-reconstruction_amd", "sparseconvnet",
                            "planExecutor.py")).read()
    assert not re.findall(r"\b(op|nop|nxt|add_op)\[", src)
