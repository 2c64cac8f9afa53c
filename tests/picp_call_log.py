"""The call log of the projective ICP's host layer.  TEST INFRASTRUCTURE ONLY.

ops.lib, ops.require_device, ops.stream, ops.Workspace and ops.check are replaced with recorders, the public functions of
the projective section of gradslam_amd/ops.py (and ProjectiveICPOdometryProvider) are driven on small CPU tensors, and
every library call they would have made is written down as text.  The library itself is loaded (that needs no GPU): its
*_bytes exports answer for real, every other export is recorded and returns 0, so no kernel runs and the outputs hold
whatever torch.empty left in them.

One case of the log:

    == <case>
    ws <key> <bytes>                      a request to the workspace
    CALL <export> <arg> ...               scalars by value, pointers as NULL / PTR, in the order of the export's argtypes
      a<i>[b] value ...                   every field of every descriptor of argument i, in the order of the FIELDS line
                                          that precedes the first descriptor of its type (nested structures dotted)
      a<i> NULL | PTR +<bytes> ...        a host table of device pointers
    RET <shapes and dtypes of what the public function returned>   or   RAISED <type>: <message>

A pointer of sequence b > 0 that addresses a slice of the tensor sequence 0's pointer addresses (SLICED below, and every
entry of a pointer table) is written as its byte distance from sequence 0's; pointers into per-sequence tensors (map
buffers, scratch, map gradients, records) are NULL or PTR.  So a grid case must not hand a pointer table two separately
allocated tensors: the list form of pixel_weights is driven with a None entry.

log() returns the text; tests/golden/picp_call_log.txt is log() at the commit before the host layer was restructured
(`python -m tests.picp_call_log FILE` writes it)."""
import contextlib
import ctypes as C
import itertools
import os
import sys

import torch

from gradslam_amd import _C, ops

B, H, W, STRIDE, NUMITERS, ROWS = 2, 6, 7, 2, 3, 9
ENV = "GRADSLAM_HIP_DETERMINISTIC_BACKWARD"
# descriptor fields that address sequence b's slice of ONE batched tensor
SLICED = {"vertex", "normal", "depth", "K16", "index", "model_pose16", "init_pose16", "out_pose16", "trace", "color",
          "model_intensity", "tape", "pose_bar16", "vertex_bar", "init_pose_bar16"}


def _addr(v):
    v = getattr(v, "value", v)
    return int(v or 0)


def _pointer(v, first=None):
    a = _addr(v)
    if not a:
        return "NULL"
    return "PTR" if not first else "%+d" % (a - first)


def _fields(s, prefix=""):
    for name, kind in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            yield from _fields(v, prefix + name + ".")
        else:
            yield prefix + name, kind, v


def _descriptor(s, first):
    """one line of a descriptor, its values in the order of the FIELDS line of its type; first: sequence 0's (None for
    sequence 0 itself)"""
    ref = {} if first is None else {n: _addr(v) for n, k, v in _fields(first) if k is C.c_void_p}
    return " ".join(_pointer(v, ref.get(name) if name.split(".")[-1] in SLICED else None) if kind is C.c_void_p
                    else repr(v) for name, kind, v in _fields(s))


class _Recorder:
    def __init__(self):
        self.lines = []
        self.real = _C.lib()
        self.legend = set()
        self.last = None

    def fields(self, s):
        """the FIELDS line of a descriptor type, written where the type first appears"""
        if type(s).__name__ not in self.legend:
            self.legend.add(type(s).__name__)
            self.lines.append("FIELDS %s %s" % (type(s).__name__, " ".join(n for n, _, _ in _fields(s))))

    def check(self, status, what):
        if status != 0 or what != self.last:   # (an export checked under its own name goes without saying)
            self.lines.append("check %s %d" % (what, status))

    # ---- ops.lib()
    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name.endswith("_bytes"):
            return fn

        def call(*args):
            assert len(args) == len(fn.argtypes), name
            head, tail = ["CALL", name], []
            for i, (kind, a) in enumerate(zip(fn.argtypes, args)):
                if kind is C.c_void_p:
                    head.append(_pointer(a))
                elif kind is C.c_float or kind is C.c_double:
                    head.append(repr(float(a)))
                elif kind in (C.c_int, C.c_int64):
                    head.append(repr(int(a)))
                elif a is None:
                    head.append("a%d=NULL" % i)
                elif isinstance(a, C.Structure):       # (a parameter block handed by reference)
                    self.fields(a)
                    head.append("a%d" % i)
                    tail.append("  a%d %s" % (i, _descriptor(a, None)))
                elif issubclass(a._type_, C.Structure):
                    self.fields(a[0])
                    head.append("a%d" % i)
                    tail += ["  a%d[%d] %s" % (i, b, _descriptor(s, a[0] if b else None)) for b, s in enumerate(a)]
                else:                                  # (a host table of device pointers)
                    head.append("a%d" % i)
                    tail.append("  a%d %s" % (i, " ".join(_pointer(p, _addr(a[0]) if b else None)
                                                          for b, p in enumerate(a))))
            self.lines.append(" ".join(head))
            self.lines += tail
            self.last = name
            return 0
        return call

    # ---- ops.Workspace
    def get(self, dev):
        return self

    def bytes(self, key, nbytes):
        self.lines.append("ws %s %d" % (key, nbytes))
        return torch.empty(int(nbytes), dtype=torch.uint8)


def _require_device(*tensors):
    for t in tensors:
        if t is not None:
            return t.device
    return None


@contextlib.contextmanager
def _recording():
    rec = _Recorder()
    saved = {k: getattr(ops, k) for k in ("lib", "require_device", "stream", "Workspace", "check")}
    ops.lib, ops.require_device, ops.stream, ops.Workspace = (lambda: rec), _require_device, (lambda dev: None), rec
    ops.check = rec.check
    env = os.environ.pop(ENV, None)
    try:
        yield rec
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        os.environ.pop(ENV, None)
        if env is not None:
            os.environ[ENV] = env


def _shapes(x):
    if x is None:
        return "None"
    if torch.is_tensor(x):
        return "%s%s" % (str(x.dtype).split(".")[-1], list(x.shape))
    return "%s(%s)" % (type(x).__name__, ", ".join(_shapes(y) for y in x))


def _inputs():
    g = torch.Generator().manual_seed(0)
    r = lambda *shape: torch.rand(shape, generator=g)   # noqa: E731
    x = dict(vertex=r(B, H, W, 3), normal=r(B, H, W, 3), depth=r(B, H, W), K=r(B, 4, 4),
             index=torch.randint(-1, ROWS, (B, H, W), generator=g), model=r(B, 4, 4), init=r(B, 4, 4),
             color=r(B, H, W, 3), intensity=r(B, H, W, 4), weights=r(B, H, W), pose_bar=r(B, 4, 4))
    # sequence 0: every row, the count on the host; sequence 1: a bound below the rows and a count on the device
    x["maps"] = [(r(ROWS, 3), r(ROWS, 3), None, None), (r(ROWS, 3), r(ROWS, 3), ROWS - 2, torch.tensor([ROWS - 3]))]
    return x


def _kw(d):
    return " ".join("%s=%s" % (k, "tensor" if torch.is_tensor(v) else "list" if isinstance(v, list) else v)
                    for k, v in d.items())


# the option sets that reach every rung of the five ladders (geometric: huber_delta, huber_k; colour: + the colour pair)
GEOMETRIC = [dict(), dict(huber_delta=0.05), dict(huber_k=1.345), dict(huber_delta=0.02, huber_k=1.345)]
COLOUR = [dict(), dict(huber_delta=0.05), dict(color_huber_delta=0.1), dict(huber_delta=0.05, color_huber_delta=0.1),
          dict(huber_k=1.345), dict(huber_k=1.345, color_huber_delta=0.1), dict(color_huber_k=1.345),
          dict(color_huber_k=1.345, huber_k=1.345, huber_delta=0.02, color_huber_delta=0.1)]


def _flag_sets(names, full):
    """all off, all on, each flag alone (full: every combination)"""
    if full:
        return [dict(zip(names, v)) for v in itertools.product((False, True), repeat=len(names))]
    sets = [dict.fromkeys(names, False), dict.fromkeys(names, True)]
    return sets + ([{n: n == m for n in names} for m in names] if len(names) > 1 else [])


def log():
    with _recording() as rec:
        _drive(rec)
    return "\n".join(rec.lines) + "\n"


def _drive(rec):
    x = _inputs()
    batch = (x["vertex"], x["normal"], x["depth"], x["K"], x["index"], x["model"], x["maps"], x["init"])
    one = (x["vertex"][0], x["normal"][0], x["depth"][0], x["K"][0], x["index"][0], x["model"][0], x["maps"][0][0],
           x["maps"][0][1], x["init"][0])
    geo = dict(stride=STRIDE, numiters=NUMITERS)
    weight_forms = [None, x["weights"], [None, x["weights"][1]]]

    def case(name, fn, *args, **kw):
        rec.lines.append("== %s %s" % (name, _kw(kw)))
        try:
            res = fn(*args, **kw)
        except Exception as e:   # noqa: BLE001
            rec.lines.append("RAISED %s: %s" % (type(e).__name__, e))
            return None
        rec.lines.append("RET " + _shapes(res))
        return res

    # ------------------------------------------------------------------------------------------- batch
    for pw, opts in itertools.product(weight_forms, GEOMETRIC):
        if isinstance(pw, list) and opts != GEOMETRIC[3]:
            continue
        for flags in _flag_sets(("return_trace", "return_scale"), full=True):
            case("batch", ops.projective_icp_batch, *batch, pixel_weights=pw, **geo, **opts, **flags)
        case("batch out", ops.projective_icp_batch, *batch, pixel_weights=pw, out=torch.empty(B, 4, 4), **geo, **opts,
             return_trace=True, return_scale=True)
    for pw in (None, x["weights"][0]):
        case("one", ops.projective_icp, *one, n_dev=torch.tensor([ROWS - 1]), pixel_weights=pw, huber_k=1.345,
             return_trace=True, return_scale=True, **geo)
        case("one", ops.projective_icp, *one, pixel_weights=pw, **geo)

    # ------------------------------------------------------------------------------------------- rows
    for pw, opts, rw in itertools.product((None, x["weights"][0]), GEOMETRIC, (False, True)):
        case("rows", ops.projective_icp_rows, *one, pixel_weights=pw, stride=STRIDE, return_weights=rw, **opts)

    # ------------------------------------------------------------------------------------------- colour batch
    cbatch = batch + (x["color"], x["intensity"])
    names = ("return_trace", "return_scale", "return_color_scale")
    for pw, opts in itertools.product(weight_forms, COLOUR):
        if isinstance(pw, list) and opts != COLOUR[7]:
            continue
        for flags in _flag_sets(names, full=False)[:1] + _flag_sets(names, full=False)[3:]:
            case("color batch", ops.projective_icp_color_batch, *cbatch, color_weight=0.3, pixel_weights=pw, **geo,
                 **opts, **flags)
        case("color batch out", ops.projective_icp_color_batch, *cbatch, color_weight=0.3, pixel_weights=pw,
             out=torch.empty(B, 4, 4), **geo, **opts, **dict.fromkeys(names, True))
    case("color batch weight 0", ops.projective_icp_color_batch, *cbatch, color_weight=0, huber_k=1.345, **geo)
    for pw in (None, x["weights"][0]):
        case("color one", ops.projective_icp_color, *one, x["color"][0], x["intensity"][0], color_weight=0.3,
             pixel_weights=pw, color_huber_k=1.345, return_trace=True, return_scale=True, return_color_scale=True, **geo)

    # ------------------------------------------------------------------------------------------- colour rows
    cone = one + (x["color"][0], x["intensity"][0])
    for pw, opts, rw in itertools.product((None, x["weights"][0]), COLOUR, (False, True)):
        case("color rows", ops.projective_icp_color_rows, *cone, color_weight=0.3, pixel_weights=pw, stride=STRIDE,
             return_weights=rw, **opts)

    # ------------------------------------------------------------------------------------------- backward
    tapes = torch.empty((B, ops.projective_icp_tape_bytes(NUMITERS)), dtype=torch.uint8)
    bwd = batch[:7] + (tapes, x["pose_bar"])
    for pw, opts, det in itertools.product(weight_forms[:2], GEOMETRIC[:3], (False, True)):
        for extra in [dict()] + ([dict(return_contributions=True)] if det else []) + \
                ([dict(want_pixel_weights=True)] if pw is not None else []):
            case("backward", ops.projective_icp_backward_batch, *bwd, pixel_weights=pw, deterministic=det, **geo, **opts,
                 **extra)
    for det, pw in itertools.product((False, True), weight_forms):
        case("backward no maps", ops.projective_icp_backward_batch, *bwd, deterministic=det, pixel_weights=pw,
             want_maps=[(False, False)] * B, want_pixel_weights=pw is not None, **geo)
        case("backward some", ops.projective_icp_backward_batch, *bwd, deterministic=det, pixel_weights=pw,
             want_vertex=False, want_init=False, want_maps=[(False, False), (False, True)], **geo)
    for env in (None, "0", "1", " +2x"):
        os.environ.pop(ENV, None)
        if env is not None:
            os.environ[ENV] = env
        case("backward env=%r" % (env,), ops.projective_icp_backward_batch, *bwd, deterministic=None, **geo)
        case("backward env=%r" % (env,), ops.projective_icp_backward_batch, *bwd, deterministic=None, huber_k=1.345,
             pixel_weights=x["weights"], want_pixel_weights=True, **geo)
    os.environ.pop(ENV, None)

    # ------------------------------------------------------------------------------------------- autograd
    def taped(name, grads, pw=None, env=None, **kw):
        """forward on the tape, then .backward(); grads: the inputs that require grad"""
        os.environ.pop(ENV, None)
        if env is not None:
            os.environ[ENV] = env
        leaf = lambda t, n: t.clone().requires_grad_(n in grads)   # noqa: E731
        v, i0 = leaf(x["vertex"], "vertex"), leaf(x["init"], "init")
        maps = [(leaf(m[0], "points%d" % b), leaf(m[1], "normals%d" % b), m[2], m[3]) for b, m in enumerate(x["maps"])]
        w = leaf(pw, "weights") if torch.is_tensor(pw) else pw   # (the list form is refused on the tape)
        res = case("taped %s env=%r grads=%s" % (name, env, ",".join(grads)), ops.projective_icp_batch, v, *batch[1:6],
                   maps, i0, differentiable=True, pixel_weights=w, **geo, **kw)
        if res is None:
            return
        T = res[0] if isinstance(res, tuple) else res
        rec.lines.append("requires_grad %s" % T.requires_grad)
        if T.requires_grad:
            T.sum().backward()
        named = [("vertex", v), ("init", i0), ("weights", w if torch.is_tensor(w) else None)] + \
            [("%s%d" % (k, b), m[j]) for b, m in enumerate(maps) for j, k in enumerate(("points", "normals"))]
        rec.lines.append("GRADS " + " ".join("%s=%s" % (n, _shapes(None if t is None else t.grad)) for n, t in named))
        os.environ.pop(ENV, None)

    every = ("vertex", "init", "points0", "normals0", "points1", "normals1")
    for pw, opts, det in itertools.product(weight_forms[:2], GEOMETRIC[:3], (False, True)):
        taped("batch", every + (("weights",) if pw is not None else ()), pw, deterministic=det, return_trace=det,
              return_scale=det, **opts)
    for pw, env in itertools.product(weight_forms[:2], (None, "0", "1")):
        taped("batch", every + (("weights",) if pw is not None else ()), pw, env=env, deterministic=None)
    for grads in (("vertex",), ("init",), ("normals1",), ("points0", "points1"), ()):
        taped("batch", grads, deterministic=True, huber_delta=0.05)
        taped("batch", grads, x["weights"], deterministic=False, huber_k=1.345)
    taped("batch", ("weights",), x["weights"], deterministic=True)
    taped("batch", ("weights",), x["weights"], deterministic=False, return_scale=True)
    taped("batch list", every, [None, x["weights"][1]])
    case("taped out", ops.projective_icp_batch, *batch, differentiable=True, out=torch.empty(B, 4, 4), **geo)
    res = case("taped one", ops.projective_icp, x["vertex"][0].clone().requires_grad_(True), *one[1:],
               pixel_weights=x["weights"][0], differentiable=True, deterministic=True, huber_k=1.345, return_scale=True,
               **geo)
    res[0].sum().backward()

    # ------------------------------------------------------------------------------------------- refusals, in order
    bad = [dict(stride=0, huber_k=-1.0), dict(huber_k=True, huber_delta=-1.0), dict(huber_delta=float("nan")),
           dict(return_scale=1, huber_k="x"), dict(deterministic=1, stride=1.5), dict(damp=0.0, angle_thresh=91),
           dict(differentiable=1), dict(pixel_weights=x["weights"][:1], stride=0), dict(pixel_weights=3),
           dict(pixel_weights=[None]), dict(pixel_weights=x["weights"].double()), dict(numiters=True),
           dict(dist_thresh=None), dict(out=torch.empty(B, 4, 3))]
    for kw in bad:
        case("refused batch", ops.projective_icp_batch, *batch, **kw)
        if "differentiable" not in kw and "out" not in kw and "return_scale" not in kw:
            case("refused backward", ops.projective_icp_backward_batch, *bwd, **kw)
        if not {"differentiable", "out", "return_scale", "numiters", "damp", "deterministic"} & set(kw):
            case("refused rows", ops.projective_icp_rows, *one, **{
                k: v[0] if k == "pixel_weights" and torch.is_tensor(v) else v for k, v in kw.items()})
    case("refused batch", ops.projective_icp_batch, *batch[:7], x["init"][:1])
    case("refused batch", ops.projective_icp_batch, *batch[:4], x["index"].int(), *batch[5:])
    case("refused batch", ops.projective_icp_batch, *batch[:6], x["maps"][:1], x["init"])
    case("refused backward", ops.projective_icp_backward_batch, *bwd, want_pixel_weights=True)
    case("refused backward", ops.projective_icp_backward_batch, *bwd, return_contributions=True, deterministic=False)
    case("refused backward", ops.projective_icp_backward_batch, *bwd[:7], tapes[:, :-1], x["pose_bar"])
    case("refused backward", ops.projective_icp_backward_batch, *bwd, want_maps=[(True, True)])
    case("refused rows", ops.projective_icp_rows, *one, return_weights=0, huber_k=-1)
    cbad = [dict(color_weight=-1.0, differentiable=True), dict(color_weight=0.0, color_huber_k=1.0),
            dict(color_weight=True), dict(color_weight=0.3, color_huber_k=-1, huber_k=-1),
            dict(color_weight=0.3, return_color_scale=0, huber_delta=-1), dict(color_weight=0.3, differentiable=True),
            dict(color_weight=0.3, huber_k=-1, huber_delta=-1), dict(color_weight=0.3, color_huber_delta=-1, stride=0),
            dict(color_weight=0.3, return_scale=0, color_huber_delta=-1)]
    for kw in cbad:
        case("refused color batch", ops.projective_icp_color_batch, *cbatch, **kw)
        if not {"differentiable", "return_scale", "return_color_scale"} & set(kw):
            case("refused color rows", ops.projective_icp_color_rows, *cone, **kw)
    case("refused color batch", ops.projective_icp_color_batch, *batch, x["color"].double(), x["intensity"],
         color_weight=0.3)
    case("refused color rows", ops.projective_icp_color_rows, *cone, color_weight=0.3, return_weights=None, stride=0)

    _drive_provider(rec, case, x)


def _drive_provider(rec, case, x):
    """ProjectiveICPOdometryProvider: its refusals, then localize in its three modes"""
    import gradslam_amd as gs
    from gradslam_amd.odometry.projicp import ProjectiveICPOdometryProvider as Provider
    for kw in (dict(pixel_weights=3), dict(differentiable=1), dict(deterministic_backward=1), dict(stride=0),
               dict(numiters=0, color_weight=-1), dict(color_weight=-1, differentiable=True),
               dict(color_weight=0.3, differentiable=True), dict(huber_delta=-1, color_huber_delta=-1),
               dict(color_huber_delta=0.1), dict(huber_k=-1, color_huber_delta=0.1), dict(color_huber_k=1.0),
               dict(color_huber_k=-1.0), dict(huber_k=True), dict(damp=0)):
        case("refused provider", Provider, **kw)
    frames = gs.RGBDImages(torch.rand(B, 1, H, W, 3), torch.rand(B, 1, H, W, 1) + 0.5,
                           torch.eye(4).expand(B, 1, 4, 4).contiguous(), torch.eye(4).expand(B, 1, 4, 4).contiguous())
    frames.vertex_map   # (the frame maps are made here, outside the cases)
    rec.lines.append("== provider")
    prev = x["init"].view(B, 1, 4, 4)
    modes = [dict(), dict(huber_delta=0.05, huber_k=1.345, stride=STRIDE, min_confidence=0.5),
             dict(differentiable=True), dict(differentiable=True, huber_k=1.345, deterministic_backward=True),
             dict(color_weight=0.3), dict(color_weight=0.3, huber_k=1.345, color_huber_k=1.345, color_huber_delta=0.1)]
    for kw, weighted in itertools.product(modes, (False, True)):
        pc = gs.Pointclouds([m[0].clone() for m in x["maps"]], [m[1].clone() for m in x["maps"]],
                            [m[0].clone() for m in x["maps"]], [m[0][:, :1].clone() for m in x["maps"]])
        if kw.get("differentiable"):
            for t in pc._buf["points"]:
                t.requires_grad_(True)
        p = Provider(numiters=NUMITERS, pixel_weights=(lambda fr: x["weights"].view(B, 1, H, W)) if weighted else None,
                     **kw)
        T = case("localize weighted=%s %s" % (weighted, _kw(kw)), p.localize, pc, frames, prev)
        if T is not None and T.requires_grad:
            T.sum().backward()
            rec.lines.append("GRADS " + " ".join(_shapes(t.grad) for t in pc._buf["points"]))
    pc = gs.Pointclouds([m[0].clone() for m in x["maps"]], [m[1].clone() for m in x["maps"]])
    case("refused localize", Provider(color_weight=0.3).localize, pc, frames, prev)
    case("refused localize", Provider(pixel_weights=lambda fr: x["weights"][0]).localize, pc, frames, prev)
    case("refused localize", Provider(pixel_weights=lambda fr: x["weights"].double()).localize, pc, frames, prev)
    case("refused localize", Provider().localize, pc, frames, prev[:1])


if __name__ == "__main__":
    text = log()
    with open(sys.argv[1], "w") as f:
        f.write(text)
    print("%d lines, %d bytes" % (text.count("\n"), len(text)))
