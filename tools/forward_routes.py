"""The route loop of tools/bench_mobilenet_forward.py and tools/bench_resnext_forward.py."""
import torch


def time_routes(model, x, reps):
    """Both routes of a packed CNN on the batch x, the fused one with check=False (no host read): two untimed calls, then
    `reps` calls timed with device events, the median.  Returns the result line's routes_bit_equal, layers, fused and
    fused_vs_layers fields."""
    res, outs = {}, {}
    for route in ("layers", "fused"):
        fn = (lambda: model(x, route="fused", check=False)) if route == "fused" else (lambda: model(x, route="layers"))
        outs[route] = fn()
        fn()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        ms = sorted(ts)[len(ts) // 2]
        res[route] = {"ms": round(ms, 3), "images_per_s": round(x.shape[0] / (ms * 1e-3), 1)}
    return {"routes_bit_equal": bool(torch.equal(outs["layers"], outs["fused"])), **res,
            "fused_vs_layers": round(res["layers"]["ms"] / res["fused"]["ms"], 2)}
