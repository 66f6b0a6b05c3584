"""The split of a built circuit into a boolean core and a field tail (zk_circuit_mixed_dims, csrc/builder.hpp: built_split) restated in
Python on top of tests/builder_pack_model.py.  Nothing here calls the library.

    SplitModel     PackModel that keeps, per wire, whether it is bit-class and its level in the core tape, and per sub-circuit where it
                   goes: "core" (one boolean operation), "cpack" (a pack over bit-class wires: gathered), "tail", "assert" (nothing)
    mixed_shape    the seven numbers of zk_circuit_mixed_dims from a SplitModel and its Finished
    split_inputs   a row of inputs in creation order -> (packed bit inputs, field inputs)
"""
import builder_model as bm
import builder_pack_model as pm

R = bm.R


class SplitModel(pm.PackModel):
    def __init__(self):
        super().__init__()
        self.bitc = [True, True]                            # per wire: bit-class
        self.level = [0, 0]                                 # per wire: level in the core tape (bit-class wires only)
        self.cat = []                                       # per sub-circuit

    def _wire(self, kind):
        self.bitc.append(kind == "bit")
        self.level.append(0)
        return super()._wire(kind)

    def sub_circuit(self, left, right, with_out=True):
        self.cat.append("tail" if with_out else "assert")
        return super().sub_circuit(left, right, with_out)

    def gate(self, kind, x, y=None):
        first_sub, first_wire = len(self.subs), len(self.kind)
        out = super().gate(kind, x, y)
        if self.bitc[x] and (kind in bm.UNARY or self.bitc[y]):
            lv = 1 + max(self.level[x], 0 if kind in bm.UNARY else self.level[y])
            for k in range(first_sub, len(self.subs)):
                self.cat[k] = "core"
            for w in range(first_wire, len(self.kind)):
                self.bitc[w] = True
                self.level[w] = lv
            if kind == "nand":
                self.level[out] = lv + 1                    # NOT of the AND
        return out

    def pack(self, bits):
        out = super().pack(bits)
        if all(self.bitc[w] for w in bits):
            self.cat[-1] = "cpack"
        return out


def mixed_shape(model, fin):
    """dict with the keys of Circuit.mixed_dims"""
    n_bit = sum(1 for k in model.kind if k == "bit")
    n_field = sum(1 for k in model.kind if k == "field")
    core_levels = [model.level[out] for (_, _, out), cat in zip(model.subs, model.cat) if cat == "core"]
    # operand of the tail per witness index: ("slot", level) | ("pack",) | ("bit",); a pack becomes a slot at its first reader
    ref = {}
    for w in range(2, len(model.kind)):
        if model.kind[w] == "field":
            ref[fin.wit[w]] = ["slot", 0]
    for (_, _, out), cat in zip(model.subs, model.cat):
        if cat == "cpack":
            ref[fin.wit[out]] = ["pack"]
        elif cat == "tail":
            ref[fin.wit[out]] = ["slot", 0]
    count = dict(ops=0, slots=sum(1 for r in ref.values() if r[0] == "slot"))
    per_level = {}

    def emit(a, b, fresh=True):
        lv = 1 + max(a, b)
        per_level[lv] = per_level.get(lv, 0) + 1
        count["ops"] += 1
        count["slots"] += fresh
        return lv

    def read(i):
        r = ref.get(i)
        if r is None:
            return 0                                        # a bit-class index
        if r[0] == "pack":
            ref[i] = r = ["slot", emit(0, 0)]               # the copy
        return r[1]

    def side(terms):
        acc = None
        for c, i in terms:
            if i == 0:
                v = 0
            elif c == 1:
                v = read(i)
            else:
                v = emit(0, read(i))
            acc = v if acc is None else emit(acc, v)
        return 0 if acc is None else acc

    for (l, r, o), cat in zip(fin.subs, model.cat):
        if cat != "tail":
            continue
        left = side(l)
        ref[o][1] = emit(left, left if l == r else side(r), fresh=False)
    return dict(n_bit_inputs=n_bit, n_field_inputs=n_field, core_ops=len(core_levels), core_levels=max(core_levels or [0]),
                tail_ops=count["ops"], tail_levels=len(per_level), tail_slots=count["slots"])


def split_inputs(model, row):
    """row: the inputs in creation order (bm.Finished.evaluate's) -> (bytes of the packed bit inputs, list of field inputs)"""
    kinds = [k for k in model.kind if k in ("bit", "field")]
    bits = [x for k, x in zip(kinds, row) if k == "bit"]
    fields = [x for k, x in zip(kinds, row) if k == "field"]
    bits += [0] * (-len(bits) % 8)
    return bm.bits_to_bytes(bits), fields
