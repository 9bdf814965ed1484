"""Cost of one evaluation batch with the metrics composed from library operators and with csrc/eval_metrics.hip
(`model.fused_metrics` off / on), B = 32, P = 20, N = 1000, part counts of `bench.representative_parts`.  One JSON line:

  c2_*          pn_transformer, everyday preset, eval mode, sample_iter 1
  global_*      B-Global on semantic data (matching + min-of-5; with a contact table), its sample_iter
  *_ms_off/on   ms per `validation_step`, both settings in ONE process, alternating windows after a warm-up; each figure
                is a host clock around a window that ends in a device synchronise, divided by its batches; the median of
                the windows is reported
  *_launches_*  device kernels of one `_calc_metrics` call (torch profiler, device-side kernel events; `*_kernels_on` names
                those of the fused path); `*_copies_*` its device-side memcpy / memset events

GPU only:  python tools/eval_rate.py [--batches 30] [--windows 5]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_rig as rig  # noqa: E402  (puts the repository root on sys.path)
from multi_part_assembly_amd import config, synthetic  # noqa: E402
from multi_part_assembly_amd.pn_transformer import build_model  # noqa: E402


def metric_launches(model, batch, fused):
    """Device kernels of ONE `_calc_metrics` call: its arguments are taken from a real `validation_step`, the call is
    repeated alone under the torch profiler, and the kernel events of the device side are counted by name.  Returns
    (kernels, {name: count}, copies): `copies` counts the device-side memcpy / memset events of the call (the runtime's
    copy and fill kernels included), which the fused path must not have."""
    from collections import Counter

    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    inner, captured = model._calc_metrics, []

    def wrapped(*a, **k):
        captured.append((a, k))
        return inner(*a, **k)

    model._calc_metrics = wrapped
    model.fused_metrics = fused
    try:
        with torch.no_grad():
            model.validation_step(batch, 0)
            del model._calc_metrics
            a, k = captured[0]
            inner(*a, **k)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                inner(*a, **k)
                torch.cuda.synchronize()
    finally:
        model.__dict__.pop("_calc_metrics", None)
        model.fused_metrics = False
    device = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    copies = [n for n in device if "memcpy" in n.lower() or "memset" in n.lower() or "copyBuffer" in n or "fillBuffer" in n]
    names = Counter(n.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split()[-1][-40:]
                    for n in device if n not in copies)
    return sum(names.values()), dict(names), len(copies)


def measure(model, batches, args):
    model.eval()
    out = {}

    def step(fused):
        def fn(i):
            model.fused_metrics = fused
            with torch.no_grad():
                model.validation_step(batches[i % len(batches)], i)
        return fn

    rig.report(out, rig.alternate({"off": step(False), "on": step(True)}, args.batches, args.windows, 5), key="ms_{name}")
    model.fused_metrics = False
    out["launches_off"], _, out["copies_off"] = metric_launches(model, batches[0], False)
    out["launches_on"], out["kernels_on"], out["copies_on"] = metric_launches(model, batches[0], True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, P, N = 32, 20, 1000
    torch.manual_seed(0)
    result = {"B": B, "P": P, "N": N, "batches_per_window": args.batches, "windows": args.windows}

    model = build_model(config.pn_transformer_everyday()).to(dev)
    for k, v in measure(model, rig.c2_batches(dev, 2, B=B, P=P, N=N, keep_num_parts=True), args).items():
        result[f"c2_{k}"] = v

    cfg = config.global_partnet_chair()
    model = build_model(cfg).to(dev)
    g = torch.Generator().manual_seed(5)
    batches = []
    for i in range(2):
        b = synthetic.make_semantic_batch(B, max_parts=P, num_points=N, seed=99 + i, device=dev)
        contact = torch.zeros(B, P, P, 4)
        contact[..., 0] = (torch.rand(B, P, P, generator=g) < 0.15).float()
        contact[..., 1:] = torch.randn(B, P, P, 3, generator=g) * 0.05
        b["contact_points"] = contact.to(dev)
        batches.append(b)
    result["global_sample_iter"] = model.sample_iter
    args.batches = max(3, args.batches // 3)
    for k, v in measure(model, batches, args).items():
        result[f"global_{k}"] = v
    rig.emit(result, None)


if __name__ == "__main__":
    main()
