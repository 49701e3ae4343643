"""What recording a trajectory costs the device-resident sampler.

One process = one mode at one size; loop_ms is the device time of the reverse loop (stats["loop_ms"] of sampler.sample, HIP
events), full-depth model, use_graph=True.  Run the modes in alternation on one box, each several times:

    python tools/measure_record_cost.py --mode return_traj --N 128 --B 1      # a list of per-step clones: works on older trees too
    python tools/measure_record_cost.py --mode none        --N 128 --B 1      # no trajectory
    python tools/measure_record_cost.py --mode reference   --N 128 --B 1      # record="reference" (fd_sample_record)
    python tools/measure_record_cost.py --mode inference   --N 128 --B 1      # wall time of a whole inference_fn(aux_traj=True) call
    python tools/measure_record_cost.py --mode metrics     --N 128 --B 1      # metrics=True (fd_backbone_metrics after the loop)

--root points at another checkout of this project (e.g. the parent commit, built) to measure that tree instead.
"""
import argparse
import json
import os
import sys
import time
import types


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("return_traj", "none", "reference", "prot", "inference", "metrics"), required=True)
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--num-t", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from se3_diffusion_amd import sampler, train_step as ts
    from se3_diffusion_amd.data import se3_diffuser
    from se3_diffusion_amd.model.score_network import ScoreNetwork
    ns = lambda d: types.SimpleNamespace(**{k: ns(v) if isinstance(v, dict) else v for k, v in d.items()})
    dev = "cuda"
    dconf = ns(dict(diffuse_trans=True, diffuse_rot=True, r3=dict(min_b=0.1, max_b=20.0, coordinate_scaling=0.1),
                    so3=dict(num_omega=1000, num_sigma=1000, min_sigma=0.1, max_sigma=1.5, schedule="logarithmic",
                             cache_dir=os.environ.get("FD_IGSO3_CACHE", "/tmp/fd_igso3_cache"), use_cached_score=False)))
    diff = se3_diffuser.SE3Diffuser(dconf)
    torch.manual_seed(0)
    model = ScoreNetwork(ts.base_model_conf(4), diff).to(dev).eval()
    kw = {"return_traj": dict(return_traj=True), "none": {}, "reference": dict(record="reference"), "prot": dict(record="prot"),
          "metrics": dict(metrics=True)}
    loop, wall = [], []
    for rep in range(a.repeats + 1):            # (the first run pays allocator growth and lazily built tables: not reported)
        gen = torch.Generator(device=dev).manual_seed(1 + rep)
        feats = sampler.init_feats(diff, a.B, a.N, dev, generator=gen)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if a.mode == "inference":
            from se3_diffusion_amd import inference
            exp = types.SimpleNamespace(model=model, diffuser=diff, _model_conf=model._model_conf,
                                        _data_conf=types.SimpleNamespace(num_t=a.num_t, min_t=0.01))
            out = inference.inference_fn(exp, feats, aux_traj=True, noise_scale=0.1, generator=gen)
            assert out["prot_traj"].shape == (a.num_t, a.B, a.N, 37, 3)
            st = {}
        else:
            st = {}
            sampler.sample(model, diff, feats, num_t=a.num_t, min_t=0.01, noise_scale=0.1, generator=gen, use_graph=True, stats=st,
                           **kw[a.mode])
        torch.cuda.synchronize()
        if rep:
            wall.append(round((time.perf_counter() - t0) * 1e3, 2))
            loop.append(round(st.get("loop_ms", float("nan")), 3))
    print(json.dumps(dict(tag=a.tag, tree=os.path.relpath(os.path.dirname(os.path.dirname(sampler.__file__))), mode=a.mode, N=a.N, B=a.B, num_t=a.num_t, loop_ms=loop, wall_ms=wall)), flush=True)


if __name__ == "__main__":
    main()
