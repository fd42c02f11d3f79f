"""What the weight-copy caches of functional.py launch, hold and return (bf16 / split8 / two-plane f16 copies of Linear and conv
weights): every entry-point call of a fixed scenario is logged at the C-ABI boundary and compared with a recorded list, the
device tables of the multi-tensor launches are decoded, and every copy is compared with a torch reference after every action.

No model: six Linear-type weights and two conv weights, the smallest that reach every branch --
  A (128, 64)   plain + transposed bf16, split8, f16           B (64, 128)   registered late (makes an optimizer's claim lapse)
  Q, K, V (64, 64)   slices of the bf16 / transposed bf16 / f16 concatenations
  P (72, 40)    the 64-padded transposed bf16 copy; has no split8 form
  C3 (64, 64, 3, 3)  bf16 forward + data-gradient layouts, split8, f16        C1 (128, 64, 1, 1)  bf16 forward layout
"""
import ctypes
import struct

import pytest
import torch

LINEAR = {"A": (128, 64), "B": (64, 128), "Q": (64, 64), "K": (64, 64), "V": (64, 64), "P": (72, 40)}
CONV = {"C3": (64, 64, 3, 3), "C1": (128, 64, 1, 1)}
MODES = ("bf16", "hpf", "mixed")
# record formats of the three table kernels (include/avsr_hip.h)
RECORDS = {"avsr_multi_cast_transpose": "<QQQiiiiiiii", "avsr_multi_weight_permute": "<QQiiiiiiii", "avsr_multi_split_pack": "<QQqq"}


def planes(w):
    """two-plane f16 image [rows][2][cols]: hi = f16(w), lo = f16((w - hi) * 2^11) (csrc/prims.h f2h_lo)"""
    hi = w.half()
    return torch.stack([hi, ((w - hi.float()) * 2048.0).half()], 1)


def bits(t):
    return t.detach().as_subclass(torch.Tensor).cpu().contiguous().view(torch.int32)


class Scenario:
    def __init__(self, dev):
        from auto_avsr_amd import _lib
        from auto_avsr_amd import functional as AF

        self.AF, self.dev, self.L = AF, dev, _lib.lib()
        torch.manual_seed(0)
        self.w = {k: torch.nn.Parameter(torch.randn(s).to(dev)) for k, s in list(LINEAR.items()) + list(CONV.items())}
        self.qkv = (self.w["Q"], self.w["K"], self.w["V"])
        self.copies = {}    # name -> tensor, as first returned by its accessor
        self.where = {}     # name -> (id, address) at registration
        self.log = None     # entries of the action in progress
        self.tables = {}    # decoded table (tuple of record strings) -> its number, in order of first appearance
        self.actions = {}   # action -> list of launch strings
        self.raw = {}       # action -> list of (entry point, table address) of the multi-tensor launches

    # ---- the log ----------------------------------------------------------------------------------------------------
    def __enter__(self):
        real = self.L.call

        def call(name, *args):
            if self.log is not None:
                blob = None
                if name in RECORDS and self.L.is_emulator:
                    blob = ctypes.string_at(args[0], args[1] * struct.calcsize(RECORDS[name]))
                self.log.append((name, args, blob))
            return real(name, *args)

        self.L.call = call
        self.AF.invalidate_weight_cache()
        return self

    def __exit__(self, *exc):
        del self.L.call
        self.AF.invalidate_weight_cache()

    def names(self):
        m = {w.data_ptr(): k for k, w in self.w.items()}
        m.update({t.data_ptr(): k for k, t in self.copies.items() if not k.startswith("QKV")})
        m[0] = "-"
        return m

    def decode(self, name, blob):
        fmt, nm = RECORDS[name], self.names()
        recs = []
        for rec in struct.iter_unpack(fmt, blob):
            nptr = 3 if name == "avsr_multi_cast_transpose" else 2
            recs.append(" ".join([nm.get(p, "?") for p in rec[:nptr]] + [str(v) for v in rec[nptr:]]))
        return self.tables.setdefault(tuple(recs), len(self.tables))

    def action(self, name, fn):
        """Run fn with the log on; file its launches under `name`."""
        self.log = []
        try:
            fn()
        finally:
            log, self.log = self.log, None
        out, raw = [], []
        for entry, args, blob in log:
            if entry in RECORDS:
                s = f"{entry} {' '.join(str(a) for a in args[1:-1])}"   # n, blocks[, max_taps]
                if blob is not None:
                    s += f" @T{self.decode(entry, blob)}"
                raw.append((entry, args[0]))
            else:
                s = entry
            out.append(s)
        assert name not in self.actions
        self.actions[name], self.raw[name] = out, raw

    # ---- the accessors ----------------------------------------------------------------------------------------------
    def bwd(self):
        """The bf16 conv copies are read by backward passes, which run with the precise flag off in every mode (functional._bwd_mode)."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            old, self.AF._state["precise"] = self.AF._state["precise"], False
            try:
                yield
            finally:
                self.AF._state["precise"] = old
        return ctx()

    def sweep(self, with_b=False):
        """One accessor of every kind; returns {name: tensor}.  Slices of a concatenation are named after their weight."""
        AF, w, got = self.AF, self.w, {}
        got["A.bf16"] = AF._w_bf16(w["A"], False)
        got["A.bf16T"] = AF._w_bf16(w["A"], True)
        got["P.bf16T"] = AF._w_bf16(w["P"], True)
        if with_b:
            got["B.bf16"] = AF._w_bf16(w["B"], False)
        got["QKV.bf16"] = AF._w_bf16_cat(self.qkv, False)
        got["QKV.bf16T"] = AF._w_bf16_cat(self.qkv, True)
        with self.bwd():
            got["C3.conv"] = AF._w_conv(w["C3"], False)
            got["C3.convT"] = AF._w_conv(w["C3"], True)
            got["C1.conv"] = AF._w_conv(w["C1"], False)
        got["A.split"] = AF._w_split(w["A"])
        assert AF._w_split(w["P"]) is None
        got["C3.split"] = AF._w_conv_split(w["C3"])
        got["A.h16"] = AF._w_h16(w["A"])
        got["QKV.h16"] = AF._w_h16_cat(self.qkv)
        got["C3.h16"] = AF._w_conv_h16(w["C3"])
        return got

    def register(self, name=None):
        """Register copies of all six kinds (logged as action `name`) and remember what the accessors returned."""
        AF, w = self.AF, self.w
        self.copies = {}
        got = {}

        def reg():
            got["A.bf16"] = AF._w_bf16(w["A"], False)
            got["A.bf16T"] = AF._w_bf16(w["A"], True)
            got["P.bf16T"] = AF._w_bf16(w["P"], True)
            got["QKV.bf16"] = AF._w_bf16_cat(self.qkv, False)
            got["QKV.bf16T"] = AF._w_bf16_cat(self.qkv, True)
            got["C3.conv"] = AF._w_conv(w["C3"], False)
            got["C3.convT"] = AF._w_conv(w["C3"], True)
            got["C1.conv"] = AF._w_conv(w["C1"], False)
            with AF.numerics("hpf"):
                got["A.split"] = AF._w_split(w["A"])
                assert AF._w_split(w["P"]) is None
                got["C3.split"] = AF._w_conv_split(w["C3"])
            with AF.numerics("mixed"):
                got["A.h16"] = AF._w_h16(w["A"])
                got["QKV.h16"] = AF._w_h16_cat(self.qkv)
                got["C3.h16"] = AF._w_conv_h16(w["C3"])
            self.adopt(got)

        if name is None:
            reg()
        else:
            self.action(name, reg)
        self.check()

    def adopt(self, got):
        """Remember the copies the accessors returned: objects, addresses, and the slices of the concatenations by weight name."""
        for k, t in got.items():
            if k.startswith("QKV"):
                for i, n in enumerate("QKV"):
                    sl = t[:, 64 * i:64 * i + 64] if k.endswith("T") else t[64 * i:64 * i + 64]
                    self.copies[n + k[3:]] = sl
            self.copies[k] = t
            self.where[k] = (id(t), t.data_ptr())

    def same_objects(self, got):
        """(c) + (d): the accessor returned the very tensor it returned at registration, and that tensor has not moved."""
        for k, t in got.items():
            assert t is self.copies[k], k
            assert self.where[k] == (id(t), t.data_ptr()), k

    # ---- contents ---------------------------------------------------------------------------------------------------
    def reference(self, name):
        AF = self.AF
        k, kind = name.split(".")
        w = self.w[k].detach()
        c = w.cpu()
        if kind == "bf16":
            return c.bfloat16()
        if kind == "bf16T":
            return c.bfloat16().t()
        if kind == "conv":
            return c.permute(0, 2, 3, 1).reshape(c.shape[0], -1).bfloat16()
        if kind == "convT":
            return c.permute(1, 2, 3, 0).reshape(c.shape[1], -1).bfloat16()
        if kind == "h16":
            return planes(c.permute(0, 2, 3, 1).reshape(c.shape[0], -1)) if c.dim() == 4 else planes(c)
        assert kind == "split"
        return bits(AF.ops.conv_weight_permute_split(w) if c.dim() == 4 else AF.ops.split_pack(w))

    def current(self, name):
        t, ref = self.copies[name], self.reference(name)
        if name.endswith(".split"):
            return torch.equal(bits(t), ref)
        t = t.detach().cpu()
        if name.endswith(".bf16T"):   # zero tail up to the 64-padded pitch (a slice of a concatenation has none)
            R = ref.shape[1]
            return torch.equal(t[:, :R], ref) and not t[:, R:].any()
        return torch.equal(t, ref)

    def check(self, stale=()):
        """(b): every copy equals its torch reference, except the ones the contract leaves stale, which must differ."""
        names = [k for k in self.copies if not k.startswith("QKV")]
        bad = [k for k in names if self.current(k) != (k not in stale)]
        assert not bad, (bad, sorted(stale))

    def nudge(self, keys=None, bump=False):
        """Change weights: in place with a version bump (a manual edit, load_state_dict) or behind the version counter (what an
        optimizer that writes through raw pointers does)."""
        with torch.no_grad():
            for k in keys or self.w:
                (self.w[k] if bump else self.w[k].data).add_(0.37)


def run(dev, mode):
    with Scenario(dev) as S:
        AF, w = S.AF, S.w
        lin_bf16 = {"A.bf16", "A.bf16T", "P.bf16T", "Q.bf16", "K.bf16", "V.bf16", "Q.bf16T", "K.bf16T", "V.bf16T"}
        S.register("register")
        assert AF._w_split(w["P"]) is None
        sizes, lin, conv = AF.cached_weight_ptrs()
        assert lin == {w[k].data_ptr() for k in "APQKV"} and conv == {w["C3"].data_ptr(), w["C1"].data_ptr()}
        assert {a: k for a, (k, _) in AF.h16_copies().items()} == {w[k].data_ptr(): (w[k].data_ptr(), tuple(w[k].shape)) for k in "AQKV"}

        def swept(name, **kw):
            res = {}
            S.action(name, lambda: res.update(S.sweep(**kw)))
            S.same_objects(res)

        with AF.numerics(mode):
            # three refreshes in a row: the same launches on the same tables
            # (the weights change behind the version counter and nobody says so: what this mode's refresh does not touch is stale,
            # and the accessors may go on returning it)
            side = {"split": {"A.split", "C3.split"}, "h16": {"A.h16", "Q.h16", "K.h16", "V.h16", "C3.h16"}}
            untouched = {"bf16": side["split"] | side["h16"], "hpf": side["h16"], "mixed": set()}[mode]
            for i in range(3):
                S.nudge()
                S.action(f"refresh {i}", AF.refresh_weight_cache)
                # the first one builds the tables that registration left unbuilt (and asks for block counts while it does);
                # from then on: the same launches on the same tables
                assert S.raw[f"refresh {i}"] == S.raw["refresh 0"]
                assert S.actions[f"refresh {i}"] == [s for s in S.actions["refresh 0"] if i == 0 or s != "avsr_weight_permute_blocks"]
                S.check(stale=untouched)
            swept("sweep after refresh")
            S.check(stale=untouched)
            if mode != "bf16":   # the precise flag is on: _w_conv hands out a fresh f32 permuted copy and leaves the cache alone
                res = []
                S.action("conv in precise mode", lambda: res.append(AF._w_conv(w["C3"], False)))
                assert res[0] is not S.copies["C3.conv"] and res[0].dtype == torch.float32
                assert torch.equal(res[0].cpu(), w["C3"].detach().cpu().permute(0, 2, 3, 1).reshape(64, -1))
            # an optimizer stepped through raw pointers
            for rewritten in (False, True):
                S.nudge()
                AF.note_optimizer_step(rewritten)
                swept(f"note_optimizer_step({rewritten}) + sweep")
                S.check()
            # edits that move the tensor version: a lone Linear weight, one slice of each concatenation, a conv weight
            S.nudge(["C3"], bump=True)
            swept("version bump of C3 + sweep")
            S.check()
            S.nudge(["A", "K"], bump=True)
            swept("version bump of A and K + sweep")
            S.check()
            # an optimizer claims the Linear bf16 copies and the f16 copies of A and Q: the refresh leaves those to it
            owner = type("Owner", (), {})()
            AF.claim_weight_casts(owner, AF.weight_cast_groups()[0])
            h16 = AF.h16_copies()
            AF.claim_h16_copies([h16[w[k].data_ptr()][0] for k in "AQ"])
            S.nudge()
            AF.note_optimizer_step(True)
            S.action("claimed: refresh", AF.refresh_weight_cache)
            swept("claimed: sweep")
            S.check(stale=lin_bf16 | {"A.h16", "Q.h16"})
            S.action("claimed: refresh again", AF.refresh_weight_cache)
            S.check(stale=lin_bf16 | {"A.h16", "Q.h16"})
            # a weight registered later changes the cache generation: the claim lapses
            res = []
            S.action("register B", lambda: res.append(AF._w_bf16(w["B"], False)))
            S.adopt({"B.bf16": res[0]})
            S.nudge()
            AF.note_optimizer_step(True)
            S.action("lapsed: refresh", AF.refresh_weight_cache)
            swept("lapsed: sweep", with_b=True)
            S.check()
            AF.claim_weight_casts(None, None)
            S.nudge()
            AF.note_optimizer_step(True)
            S.action("unclaimed: refresh", AF.refresh_weight_cache)
            swept("unclaimed: sweep", with_b=True)
            S.check()
            del owner
        AF.invalidate_weight_cache()
        assert AF.cached_weight_ptrs()[1:] == (set(), set()) and AF.h16_copies() == {} and AF.weight_cast_groups()[1] == []
        assert AF.cached_weight_ptrs()[0][0] == sizes[0] + 1
        old = dict(S.copies)
        S.register("register again")
        assert all(S.copies[k] is not old[k] for k in old if k != "B.bf16")
        with AF.numerics(mode):
            S.action("refresh after re-registration", AF.refresh_weight_cache)
            swept("sweep after re-registration")
        S.check()
        return S.actions, {n: t for t, n in S.tables.items()}


@pytest.mark.parametrize("mode", MODES)
def test_weight_copy_launches(dev, mode):
    actions, tables = run(dev, mode)
    exp_actions, exp_tables = EXPECTED[mode]
    on_emu = dev.type == "cpu"
    for name, launches in actions.items():
        want = exp_actions[name] if on_emu else [s.split(" @T")[0] for s in exp_actions[name]]
        assert launches == want, (mode, name, launches, want)
    assert list(actions) == list(exp_actions)
    if on_emu:
        assert tables == exp_tables


@pytest.mark.gpu
def test_captured_refresh_launches_kernels_only():
    """A refresh_weight_cache() of the mixed mode captured in a hipGraph, replayed after every weight changed in place: all
    copies are current again -- the capture holds kernels only, reading tables and writing copies that have not moved."""
    dev = torch.device("cuda:0")
    from auto_avsr_amd import _lib

    _lib._lib = None
    with Scenario(dev) as S:
        AF = S.AF
        S.register()
        with AF.numerics("mixed"):
            AF.refresh_weight_cache()   # builds every table (host-to-device copies) outside the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                AF.refresh_weight_cache()
        S.check()
        S.nudge()
        stale = [k for k in S.copies if not k.startswith("QKV") and S.current(k)]
        assert not stale, stale
        graph.replay()
        torch.cuda.synchronize()
        S.check()


# recorded from the caches as they stood before they were unified: per mode, ({action: launches}, {table number: decoded records})
EXPECTED = {'bf16': ({'register': ['avsr_scale_dropout',
                        'avsr_transpose_cast',
                        'avsr_transpose_cast',
                        'avsr_multi_cast_transpose 5 7 @T0',
                        'avsr_multi_cast_transpose 5 7 @T1',
                        'avsr_conv_weight_permute',
                        'avsr_conv_weight_permute',
                        'avsr_conv_weight_permute',
                        'avsr_split_pack',
                        'avsr_conv_weight_permute',
                        'avsr_multi_cast_transpose 1 2 @T2',
                        'avsr_multi_cast_transpose 1 1 @T3',
                        'avsr_multi_cast_transpose 1 1 @T4',
                        'avsr_multi_cast_transpose 1 1 @T5',
                        'avsr_weight_permute_blocks',
                        'avsr_multi_weight_permute 1 8 9 @T6'],
           'refresh 0': ['avsr_weight_permute_blocks',
                         'avsr_weight_permute_blocks',
                         'avsr_weight_permute_blocks',
                         'avsr_multi_weight_permute 3 32 9 @T7',
                         'avsr_multi_cast_transpose 5 7 @T1'],
           'refresh 1': ['avsr_multi_weight_permute 3 32 9 @T7', 'avsr_multi_cast_transpose 5 7 @T1'],
           'refresh 2': ['avsr_multi_weight_permute 3 32 9 @T7', 'avsr_multi_cast_transpose 5 7 @T1'],
           'sweep after refresh': [],
           'note_optimizer_step(False) + sweep': ['avsr_multi_weight_permute 3 32 9 @T7',
                                                  'avsr_multi_cast_transpose 5 7 @T1',
                                                  'avsr_weight_permute_blocks',
                                                  'avsr_multi_weight_permute 1 8 9 @T8',
                                                  'avsr_multi_split_pack 1 4 @T9',
                                                  'avsr_multi_weight_permute 1 8 9 @T6',
                                                  'avsr_multi_cast_transpose 4 5 @T10'],
           'note_optimizer_step(True) + sweep': ['avsr_multi_weight_permute 3 32 9 @T7',
                                                 'avsr_multi_cast_transpose 5 7 @T1',
                                                 'avsr_multi_weight_permute 1 8 9 @T8',
                                                 'avsr_multi_split_pack 1 4 @T9',
                                                 'avsr_multi_weight_permute 1 8 9 @T6',
                                                 'avsr_multi_cast_transpose 4 5 @T10'],
           'version bump of C3 + sweep': ['avsr_conv_weight_permute',
                                          'avsr_conv_weight_permute',
                                          'avsr_conv_weight_permute',
                                          'avsr_multi_weight_permute 1 8 9 @T6'],
           'version bump of A and K + sweep': ['avsr_scale_dropout',
                                               'avsr_transpose_cast',
                                               'avsr_multi_weight_permute 3 32 9 @T7',
                                               'avsr_multi_cast_transpose 5 7 @T1',
                                               'avsr_split_pack',
                                               'avsr_multi_cast_transpose 1 2 @T2',
                                               'avsr_multi_cast_transpose 1 1 @T4'],
           'claimed: refresh': ['avsr_multi_weight_permute 3 32 9 @T7'],
           'claimed: sweep': ['avsr_multi_weight_permute 1 8 9 @T8',
                              'avsr_multi_split_pack 1 4 @T9',
                              'avsr_multi_weight_permute 1 8 9 @T6',
                              'avsr_multi_cast_transpose 2 2 @T11'],
           'claimed: refresh again': ['avsr_multi_weight_permute 3 32 9 @T7'],
           'register B': ['avsr_scale_dropout'],
           'lapsed: refresh': ['avsr_multi_weight_permute 3 32 9 @T7', 'avsr_multi_cast_transpose 6 9 @T12'],
           'lapsed: sweep': ['avsr_multi_weight_permute 1 8 9 @T8',
                             'avsr_multi_split_pack 1 4 @T9',
                             'avsr_multi_weight_permute 1 8 9 @T6',
                             'avsr_multi_cast_transpose 4 5 @T10'],
           'unclaimed: refresh': ['avsr_multi_weight_permute 3 32 9 @T7', 'avsr_multi_cast_transpose 6 9 @T12'],
           'unclaimed: sweep': ['avsr_multi_weight_permute 1 8 9 @T8',
                                'avsr_multi_split_pack 1 4 @T9',
                                'avsr_multi_weight_permute 1 8 9 @T6',
                                'avsr_multi_cast_transpose 4 5 @T10'],
           'register again': ['avsr_scale_dropout',
                              'avsr_transpose_cast',
                              'avsr_transpose_cast',
                              'avsr_multi_cast_transpose 5 7 @T0',
                              'avsr_multi_cast_transpose 5 7 @T1',
                              'avsr_conv_weight_permute',
                              'avsr_conv_weight_permute',
                              'avsr_conv_weight_permute',
                              'avsr_split_pack',
                              'avsr_conv_weight_permute',
                              'avsr_multi_cast_transpose 1 2 @T2',
                              'avsr_multi_cast_transpose 1 1 @T3',
                              'avsr_multi_cast_transpose 1 1 @T4',
                              'avsr_multi_cast_transpose 1 1 @T5',
                              'avsr_weight_permute_blocks',
                              'avsr_multi_weight_permute 1 8 9 @T6'],
           'refresh after re-registration': ['avsr_weight_permute_blocks',
                                             'avsr_weight_permute_blocks',
                                             'avsr_weight_permute_blocks',
                                             'avsr_multi_weight_permute 3 32 9 @T7',
                                             'avsr_multi_cast_transpose 5 7 @T1'],
           'sweep after re-registration': []},
          {0: ('A A.bf16 A.bf16T 128 64 128 0 1 128 0 0',
               'P - P.bf16T 72 40 128 2 1 128 0 0',
               'Q Q.bf16 - 64 64 0 4 1 0 0 0',
               'K K.bf16 - 64 64 0 5 1 0 0 0',
               'V V.bf16 - 64 64 0 6 1 0 0 0'),
           1: ('A A.bf16 A.bf16T 128 64 128 0 1 128 0 0',
               'P - P.bf16T 72 40 128 2 1 128 0 0',
               'Q Q.bf16 Q.bf16T 64 64 192 4 1 64 0 0',
               'K K.bf16 K.bf16T 64 64 192 5 1 64 0 0',
               'V V.bf16 V.bf16T 64 64 192 6 1 64 0 0'),
           2: ('A A.h16 - 128 64 0 0 1 0 2 0',),
           3: ('Q Q.h16 - 64 64 0 0 1 0 2 0',),
           4: ('K K.h16 - 64 64 0 0 1 0 2 0',),
           5: ('V V.h16 - 64 64 0 0 1 0 2 0',),
           6: ('C3 C3.h16 64 64 9 0 0 2 0 0',),
           7: ('C3 C3.conv 64 64 9 0 0 0 0 0', 'C3 C3.convT 64 64 9 1 8 0 0 0', 'C1 C1.conv 128 64 1 0 16 0 0 0'),
           8: ('C3 C3.split 64 64 9 0 0 3 0 0',),
           9: ('A A.split 1024 0',),
           10: ('A A.h16 - 128 64 0 0 1 0 2 0', 'Q Q.h16 - 64 64 0 2 1 0 2 0', 'K K.h16 - 64 64 0 3 1 0 2 0', 'V V.h16 - 64 64 0 4 1 0 2 0'),
           11: ('K K.h16 - 64 64 0 0 1 0 2 0', 'V V.h16 - 64 64 0 1 1 0 2 0'),
           12: ('A A.bf16 A.bf16T 128 64 128 0 1 128 0 0',
                'P - P.bf16T 72 40 128 2 1 128 0 0',
                'Q Q.bf16 Q.bf16T 64 64 192 4 1 64 0 0',
                'K K.bf16 K.bf16T 64 64 192 5 1 64 0 0',
                'V V.bf16 V.bf16T 64 64 192 6 1 64 0 0',
                'B B.bf16 - 64 128 0 7 2 0 0 0')}),
 'hpf': ({'register': ['avsr_scale_dropout',
                       'avsr_transpose_cast',
                       'avsr_transpose_cast',
                       'avsr_multi_cast_transpose 5 7 @T0',
                       'avsr_multi_cast_transpose 5 7 @T1',
                       'avsr_conv_weight_permute',
                       'avsr_conv_weight_permute',
                       'avsr_conv_weight_permute',
                       'avsr_split_pack',
                       'avsr_conv_weight_permute',
                       'avsr_multi_cast_transpose 1 2 @T2',
                       'avsr_multi_cast_transpose 1 1 @T3',
                       'avsr_multi_cast_transpose 1 1 @T4',
                       'avsr_multi_cast_transpose 1 1 @T5',
                       'avsr_weight_permute_blocks',
                       'avsr_multi_weight_permute 1 8 9 @T6'],
          'refresh 0': ['avsr_weight_permute_blocks',
                        'avsr_weight_permute_blocks',
                        'avsr_weight_permute_blocks',
                        'avsr_multi_weight_permute 3 32 9 @T7',
                        'avsr_weight_permute_blocks',
                        'avsr_multi_weight_permute 1 8 9 @T8',
                        'avsr_multi_split_pack 1 4 @T9',
                        'avsr_multi_cast_transpose 5 7 @T1'],
          'refresh 1': ['avsr_multi_weight_permute 3 32 9 @T7',
                        'avsr_multi_weight_permute 1 8 9 @T8',
                        'avsr_multi_split_pack 1 4 @T9',
                        'avsr_multi_cast_transpose 5 7 @T1'],
          'refresh 2': ['avsr_multi_weight_permute 3 32 9 @T7',
                        'avsr_multi_weight_permute 1 8 9 @T8',
                        'avsr_multi_split_pack 1 4 @T9',
                        'avsr_multi_cast_transpose 5 7 @T1'],
          'sweep after refresh': [],
          'conv in precise mode': ['avsr_conv_weight_permute'],
          'note_optimizer_step(False) + sweep': ['avsr_multi_weight_permute 3 32 9 @T7',
                                                 'avsr_multi_weight_permute 1 8 9 @T8',
                                                 'avsr_multi_split_pack 1 4 @T9',
                                                 'avsr_multi_cast_transpose 5 7 @T1',
                                                 'avsr_multi_weight_permute 1 8 9 @T6',
                                                 'avsr_multi_cast_transpose 4 5 @T10'],
          'note_optimizer_step(True) + sweep': ['avsr_multi_weight_permute 3 32 9 @T7',
                                                'avsr_multi_weight_permute 1 8 9 @T8',
                                                'avsr_multi_split_pack 1 4 @T9',
                                                'avsr_multi_cast_transpose 5 7 @T1',
                                                'avsr_multi_weight_permute 1 8 9 @T6',
                                                'avsr_multi_cast_transpose 4 5 @T10'],
          'version bump of C3 + sweep': ['avsr_conv_weight_permute',
                                         'avsr_conv_weight_permute',
                                         'avsr_conv_weight_permute',
                                         'avsr_multi_weight_permute 1 8 9 @T6'],
          'version bump of A and K + sweep': ['avsr_scale_dropout',
                                              'avsr_transpose_cast',
                                              'avsr_multi_weight_permute 3 32 9 @T7',
                                              'avsr_multi_weight_permute 1 8 9 @T8',
                                              'avsr_multi_split_pack 1 4 @T9',
                                              'avsr_multi_cast_transpose 5 7 @T1',
                                              'avsr_multi_cast_transpose 1 2 @T2',
                                              'avsr_multi_cast_transpose 1 1 @T4'],
          'claimed: refresh': ['avsr_multi_weight_permute 3 32 9 @T7', 'avsr_multi_weight_permute 1 8 9 @T8', 'avsr_multi_split_pack 1 4 @T9'],
          'claimed: sweep': ['avsr_multi_weight_permute 1 8 9 @T6', 'avsr_multi_cast_transpose 2 2 @T11'],
          'claimed: refresh again': ['avsr_multi_weight_permute 3 32 9 @T7', 'avsr_multi_weight_permute 1 8 9 @T8', 'avsr_multi_split_pack 1 4 @T9'],
          'register B': ['avsr_scale_dropout'],
          'lapsed: refresh': ['avsr_multi_weight_permute 3 32 9 @T7',
                              'avsr_multi_weight_permute 1 8 9 @T8',
                              'avsr_multi_split_pack 1 4 @T9',
                              'avsr_multi_cast_transpose 6 9 @T12'],
          'lapsed: sweep': ['avsr_multi_weight_permute 1 8 9 @T6', 'avsr_multi_cast_transpose 4 5 @T10'],
          'unclaimed: refresh': ['avsr_multi_weight_permute 3 32 9 @T7',
                                 'avsr_multi_weight_permute 1 8 9 @T8',
                                 'avsr_multi_split_pack 1 4 @T9',
                                 'avsr_multi_cast_transpose 6 9 @T12'],
          'unclaimed: sweep': ['avsr_multi_weight_permute 1 8 9 @T6', 'avsr_multi_cast_transpose 4 5 @T10'],
          'register again': ['avsr_scale_dropout',
                             'avsr_transpose_cast',
                             'avsr_transpose_cast',
                             'avsr_multi_cast_transpose 5 7 @T0',
                             'avsr_multi_cast_transpose 5 7 @T1',
                             'avsr_conv_weight_permute',
                             'avsr_conv_weight_permute',
                             'avsr_conv_weight_permute',
                             'avsr_split_pack',
                             'avsr_conv_weight_permute',
                             'avsr_multi_cast_transpose 1 2 @T2',
                             'avsr_multi_cast_transpose 1 1 @T3',
                             'avsr_multi_cast_transpose 1 1 @T4',
                             'avsr_multi_cast_transpose 1 1 @T5',
                             'avsr_weight_permute_blocks',
                             'avsr_multi_weight_permute 1 8 9 @T6'],
          'refresh after re-registration': ['avsr_weight_permute_blocks',
                                            'avsr_weight_permute_blocks',
                                            'avsr_weight_permute_blocks',
                                            'avsr_multi_weight_permute 3 32 9 @T7',
                                            'avsr_weight_permute_blocks',
                                            'avsr_multi_weight_permute 1 8 9 @T8',
                                            'avsr_multi_split_pack 1 4 @T9',
                                            'avsr_multi_cast_transpose 5 7 @T1'],
          'sweep after re-registration': []},
         {0: ('A A.bf16 A.bf16T 128 64 128 0 1 128 0 0',
              'P - P.bf16T 72 40 128 2 1 128 0 0',
              'Q Q.bf16 - 64 64 0 4 1 0 0 0',
              'K K.bf16 - 64 64 0 5 1 0 0 0',
              'V V.bf16 - 64 64 0 6 1 0 0 0'),
          1: ('A A.bf16 A.bf16T 128 64 128 0 1 128 0 0',
              'P - P.bf16T 72 40 128 2 1 128 0 0',
              'Q Q.bf16 Q.bf16T 64 64 192 4 1 64 0 0',
              'K K.bf16 K.bf16T 64 64 192 5 1 64 0 0',
              'V V.bf16 V.bf16T 64 64 192 6 1 64 0 0'),
          2: ('A A.h16 - 128 64 0 0 1 0 2 0',),
          3: ('Q Q.h16 - 64 64 0 0 1 0 2 0',),
          4: ('K K.h16 - 64 64 0 0 1 0 2 0',),
          5: ('V V.h16 - 64 64 0 0 1 0 2 0',),
          6: ('C3 C3.h16 64 64 9 0 0 2 0 0',),
          7: ('C3 C3.conv 64 64 9 0 0 0 0 0', 'C3 C3.convT 64 64 9 1 8 0 0 0', 'C1 C1.conv 128 64 1 0 16 0 0 0'),
          8: ('C3 C3.split 64 64 9 0 0 3 0 0',),
          9: ('A A.split 1024 0',),
          10: ('A A.h16 - 128 64 0 0 1 0 2 0', 'Q Q.h16 - 64 64 0 2 1 0 2 0', 'K K.h16 - 64 64 0 3 1 0 2 0', 'V V.h16 - 64 64 0 4 1 0 2 0'),
          11: ('K K.h16 - 64 64 0 0 1 0 2 0', 'V V.h16 - 64 64 0 1 1 0 2 0'),
          12: ('A A.bf16 A.bf16T 128 64 128 0 1 128 0 0',
               'P - P.bf16T 72 40 128 2 1 128 0 0',
               'Q Q.bf16 Q.bf16T 64 64 192 4 1 64 0 0',
               'K K.bf16 K.bf16T 64 64 192 5 1 64 0 0',
               'V V.bf16 V.bf16T 64 64 192 6 1 64 0 0',
               'B B.bf16 - 64 128 0 7 2 0 0 0')}),
 'mixed': ({'register': ['avsr_scale_dropout',
                         'avsr_transpose_cast',
                         'avsr_transpose_cast',
                         'avsr_multi_cast_transpose 5 7 @T0',
                         'avsr_multi_cast_transpose 5 7 @T1',
                         'avsr_conv_weight_permute',
                         'avsr_conv_weight_permute',
                         'avsr_conv_weight_permute',
                         'avsr_split_pack',
                         'avsr_conv_weight_permute',
                         'avsr_multi_cast_transpose 1 2 @T2',
                         'avsr_multi_cast_transpose 1 1 @T3',
                         'avsr_multi_cast_transpose 1 1 @T4',
                         'avsr_multi_cast_transpose 1 1 @T5',
                         'avsr_weight_permute_blocks',
                         'avsr_multi_weight_permute 1 8 9 @T6'],
            'refresh 0': ['avsr_weight_permute_blocks',
                          'avsr_weight_permute_blocks',
                          'avsr_weight_permute_blocks',
                          'avsr_multi_weight_permute 3 32 9 @T7',
                          'avsr_weight_permute_blocks',
                          'avsr_multi_weight_permute 1 8 9 @T8',
                          'avsr_multi_split_pack 1 4 @T9',
                          'avsr_multi_weight_permute 1 8 9 @T6',
                          'avsr_multi_cast_transpose 4 5 @T10',
                          'avsr_multi_cast_transpose 5 7 @T1'],
            'refresh 1': ['avsr_multi_weight_permute 3 32 9 @T7',
                          'avsr_multi_weight_permute 1 8 9 @T8',
                          'avsr_multi_split_pack 1 4 @T9',
                          'avsr_multi_weight_permute 1 8 9 @T6',
                          'avsr_multi_cast_transpose 4 5 @T10',
                          'avsr_multi_cast_transpose 5 7 @T1'],
            'refresh 2': ['avsr_multi_weight_permute 3 32 9 @T7',
                          'avsr_multi_weight_permute 1 8 9 @T8',
                          'avsr_multi_split_pack 1 4 @T9',
                          'avsr_multi_weight_permute 1 8 9 @T6',
                          'avsr_multi_cast_transpose 4 5 @T10',
                          'avsr_multi_cast_transpose 5 7 @T1'],
            'sweep after refresh': [],
            'conv in precise mode': ['avsr_conv_weight_permute'],
            'note_optimizer_step(False) + sweep': ['avsr_multi_weight_permute 3 32 9 @T7',
                                                   'avsr_multi_weight_permute 1 8 9 @T8',
                                                   'avsr_multi_split_pack 1 4 @T9',
                                                   'avsr_multi_weight_permute 1 8 9 @T6',
                                                   'avsr_multi_cast_transpose 4 5 @T10',
                                                   'avsr_multi_cast_transpose 5 7 @T1'],
            'note_optimizer_step(True) + sweep': ['avsr_multi_weight_permute 3 32 9 @T7',
                                                  'avsr_multi_weight_permute 1 8 9 @T8',
                                                  'avsr_multi_split_pack 1 4 @T9',
                                                  'avsr_multi_weight_permute 1 8 9 @T6',
                                                  'avsr_multi_cast_transpose 4 5 @T10',
                                                  'avsr_multi_cast_transpose 5 7 @T1'],
            'version bump of C3 + sweep': ['avsr_conv_weight_permute',
                                           'avsr_conv_weight_permute',
                                           'avsr_conv_weight_permute',
                                           'avsr_multi_weight_permute 1 8 9 @T6'],
            'version bump of A and K + sweep': ['avsr_scale_dropout',
                                                'avsr_transpose_cast',
                                                'avsr_multi_weight_permute 3 32 9 @T7',
                                                'avsr_multi_weight_permute 1 8 9 @T8',
                                                'avsr_multi_split_pack 1 4 @T9',
                                                'avsr_multi_weight_permute 1 8 9 @T6',
                                                'avsr_multi_cast_transpose 4 5 @T10',
                                                'avsr_multi_cast_transpose 5 7 @T1'],
            'claimed: refresh': ['avsr_multi_weight_permute 3 32 9 @T7',
                                 'avsr_multi_weight_permute 1 8 9 @T8',
                                 'avsr_multi_split_pack 1 4 @T9',
                                 'avsr_multi_weight_permute 1 8 9 @T6',
                                 'avsr_multi_cast_transpose 2 2 @T11'],
            'claimed: sweep': [],
            'claimed: refresh again': ['avsr_multi_weight_permute 3 32 9 @T7',
                                       'avsr_multi_weight_permute 1 8 9 @T8',
                                       'avsr_multi_split_pack 1 4 @T9',
                                       'avsr_multi_weight_permute 1 8 9 @T6',
                                       'avsr_multi_cast_transpose 2 2 @T11'],
            'register B': ['avsr_scale_dropout'],
            'lapsed: refresh': ['avsr_multi_weight_permute 3 32 9 @T7',
                                'avsr_multi_weight_permute 1 8 9 @T8',
                                'avsr_multi_split_pack 1 4 @T9',
                                'avsr_multi_weight_permute 1 8 9 @T6',
                                'avsr_multi_cast_transpose 4 5 @T10',
                                'avsr_multi_cast_transpose 6 9 @T12'],
            'lapsed: sweep': [],
            'unclaimed: refresh': ['avsr_multi_weight_permute 3 32 9 @T7',
                                   'avsr_multi_weight_permute 1 8 9 @T8',
                                   'avsr_multi_split_pack 1 4 @T9',
                                   'avsr_multi_weight_permute 1 8 9 @T6',
                                   'avsr_multi_cast_transpose 4 5 @T10',
                                   'avsr_multi_cast_transpose 6 9 @T12'],
            'unclaimed: sweep': [],
            'register again': ['avsr_scale_dropout',
                               'avsr_transpose_cast',
                               'avsr_transpose_cast',
                               'avsr_multi_cast_transpose 5 7 @T0',
                               'avsr_multi_cast_transpose 5 7 @T1',
                               'avsr_conv_weight_permute',
                               'avsr_conv_weight_permute',
                               'avsr_conv_weight_permute',
                               'avsr_split_pack',
                               'avsr_conv_weight_permute',
                               'avsr_multi_cast_transpose 1 2 @T2',
                               'avsr_multi_cast_transpose 1 1 @T3',
                               'avsr_multi_cast_transpose 1 1 @T4',
                               'avsr_multi_cast_transpose 1 1 @T5',
                               'avsr_weight_permute_blocks',
                               'avsr_multi_weight_permute 1 8 9 @T6'],
            'refresh after re-registration': ['avsr_weight_permute_blocks',
                                              'avsr_weight_permute_blocks',
                                              'avsr_weight_permute_blocks',
                                              'avsr_multi_weight_permute 3 32 9 @T7',
                                              'avsr_weight_permute_blocks',
                                              'avsr_multi_weight_permute 1 8 9 @T8',
                                              'avsr_multi_split_pack 1 4 @T9',
                                              'avsr_multi_weight_permute 1 8 9 @T6',
                                              'avsr_multi_cast_transpose 4 5 @T10',
                                              'avsr_multi_cast_transpose 5 7 @T1'],
            'sweep after re-registration': []},
           {0: ('A A.bf16 A.bf16T 128 64 128 0 1 128 0 0',
                'P - P.bf16T 72 40 128 2 1 128 0 0',
                'Q Q.bf16 - 64 64 0 4 1 0 0 0',
                'K K.bf16 - 64 64 0 5 1 0 0 0',
                'V V.bf16 - 64 64 0 6 1 0 0 0'),
            1: ('A A.bf16 A.bf16T 128 64 128 0 1 128 0 0',
                'P - P.bf16T 72 40 128 2 1 128 0 0',
                'Q Q.bf16 Q.bf16T 64 64 192 4 1 64 0 0',
                'K K.bf16 K.bf16T 64 64 192 5 1 64 0 0',
                'V V.bf16 V.bf16T 64 64 192 6 1 64 0 0'),
            2: ('A A.h16 - 128 64 0 0 1 0 2 0',),
            3: ('Q Q.h16 - 64 64 0 0 1 0 2 0',),
            4: ('K K.h16 - 64 64 0 0 1 0 2 0',),
            5: ('V V.h16 - 64 64 0 0 1 0 2 0',),
            6: ('C3 C3.h16 64 64 9 0 0 2 0 0',),
            7: ('C3 C3.conv 64 64 9 0 0 0 0 0', 'C3 C3.convT 64 64 9 1 8 0 0 0', 'C1 C1.conv 128 64 1 0 16 0 0 0'),
            8: ('C3 C3.split 64 64 9 0 0 3 0 0',),
            9: ('A A.split 1024 0',),
            10: ('A A.h16 - 128 64 0 0 1 0 2 0', 'Q Q.h16 - 64 64 0 2 1 0 2 0', 'K K.h16 - 64 64 0 3 1 0 2 0', 'V V.h16 - 64 64 0 4 1 0 2 0'),
            11: ('K K.h16 - 64 64 0 0 1 0 2 0', 'V V.h16 - 64 64 0 1 1 0 2 0'),
            12: ('A A.bf16 A.bf16T 128 64 128 0 1 128 0 0',
                 'P - P.bf16T 72 40 128 2 1 128 0 0',
                 'Q Q.bf16 Q.bf16T 64 64 192 4 1 64 0 0',
                 'K K.bf16 K.bf16T 64 64 192 5 1 64 0 0',
                 'V V.bf16 V.bf16T 64 64 192 6 1 64 0 0',
                 'B B.bf16 - 64 128 0 7 2 0 0 0')})}
