"""Shared by tools/ray_query_bench.py --sorted and tools/shade_rays_bench.py --sorted: one shuffled batch timed three ways in the same
run — (a) as it is, (b) order + gather + call + scatter as one region, (c) the parts of (b) one by one — with the image-order batch
beside them. Every figure is the median over `reps` launches bracketed by HIP events on one stream, after `warmup` uncounted ones.
The unsorted leg is timed three times (before, between and after the sorted legs): the spread of its medians is what a difference
has to exceed to mean anything. After every timed launch of the sorted region its answers are compared, byte for byte, with the
unsorted answers to the same batch."""
import statistics


def sorted_legs(pkg, ctx, torch, stream, n, d_image, d_shuffled, d_keys_image, d_keys_shuffled, out_bytes, call, reps, warmup, shading):
    """call(d_rays_ptr, d_keys_ptr or None, d_out_ptr) queues one of the five _device entries on `stream`. Returns the JSON row."""
    s = stream.cuda_stream
    u8 = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    d_order, d_sorted, d_skeys = u8(4 * n), u8(32 * n), u8(4 * n)
    d_ref, d_tmp, d_sout, d_back = u8(out_bytes * n), u8(out_bytes * n), u8(out_bytes * n), u8(out_bytes * n)
    keyed = d_keys_shuffled is not None
    kp = lambda t: t.data_ptr() if keyed else None

    def status():
        """a shading entry must be complete; warm-up launches may report capacity once per recursion level"""
        if not shading:
            return True
        try:
            ctx.frame_status()
            return True
        except pkg.RtuError as err:
            if err.code != pkg.RTU_ERR_CAPACITY:
                raise
            return False

    def order():
        ctx.ray_order_device(d_shuffled.data_ptr(), n, d_order.data_ptr(), s)

    def gather():
        ctx.permute_device(d_shuffled.data_ptr(), d_sorted.data_ptr(), d_order.data_ptr(), n, 32, False, s)
        if keyed:
            ctx.permute_device(d_keys_shuffled.data_ptr(), d_skeys.data_ptr(), d_order.data_ptr(), n, 4, False, s)

    def scatter():
        ctx.permute_device(d_sout.data_ptr(), d_back.data_ptr(), d_order.data_ptr(), n, out_bytes, True, s)

    def region():
        order()
        gather()
        call(d_sorted.data_ptr(), kp(d_skeys), d_sout.data_ptr())
        scatter()

    def timed(fn, after=None):
        for _ in range(warmup + (8 if shading else 0)):
            fn()
            status()
        stream.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if not status():
                raise RuntimeError("a timed launch was incomplete")
            ms.append(e0.elapsed_time(e1))
            if after:
                after()
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    # the unsorted answers to the shuffled batch: what every sorted launch has to reproduce
    for _ in range(9 if shading else 1):
        call(d_shuffled.data_ptr(), kp(d_keys_shuffled), d_ref.data_ptr())
        stream.synchronize()
        if status():
            break
    equal = []
    row = {"rays": int(n)}
    row["image_order"] = timed(lambda: call(d_image.data_ptr(), kp(d_keys_image), d_tmp.data_ptr()))
    unsorted = [timed(lambda: call(d_shuffled.data_ptr(), kp(d_keys_shuffled), d_tmp.data_ptr()))]
    row["sorted_region"] = timed(region, lambda: equal.append(bool(torch.equal(d_back, d_ref))))
    unsorted.append(timed(lambda: call(d_shuffled.data_ptr(), kp(d_keys_shuffled), d_tmp.data_ptr())))
    parts = {"order": timed(order), "gather": timed(gather),
             "call_on_sorted": timed(lambda: call(d_sorted.data_ptr(), kp(d_skeys), d_sout.data_ptr())), "scatter": timed(scatter)}
    unsorted.append(timed(lambda: call(d_shuffled.data_ptr(), kp(d_keys_shuffled), d_tmp.data_ptr())))
    meds = [u["median_ms"] for u in unsorted]
    row["shuffled"] = {"median_ms": statistics.median(meds), "medians_ms": meds, "spread_ms": max(meds) - min(meds),
                       "min_ms": min(u["min_ms"] for u in unsorted), "max_ms": max(u["max_ms"] for u in unsorted)}
    row["parts"] = parts
    row["sort_cost_ms"] = parts["order"]["median_ms"] + parts["gather"]["median_ms"] + parts["scatter"]["median_ms"]
    row["equal_bytes_in_every_timed_launch"] = bool(equal) and all(equal)
    row["gain_ms"] = row["shuffled"]["median_ms"] - row["sorted_region"]["median_ms"]
    row["sorted_wins"] = row["gain_ms"] > row["shuffled"]["spread_ms"]
    return row
