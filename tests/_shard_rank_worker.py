"""One rank of a multi-rank main.py run, as a fresh process (tests/test_shard_gpu.py starts one per rank):

    python _shard_rank_worker.py RANK WORLD PORT OUT_PREFIX  main.py-arguments...

With fewer GPUs than ranks the ranks share cuda:0 and exchange through gloo, which accepts device tensors (as the two-rank
engine test of tests/test_dist_gpu.py does); with enough GPUs it is one rank per GPU over RCCL.  Everything above the
transport is what a multi-GPU run executes.  Writes OUT_PREFIX.json (main()'s result) and, after a training run,
OUT_PREFIX.pt (the replica's flat parameter buffer)."""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nbdt_path  # noqa: E402

nbdt_path.add()


def run(rank, world, port, prefix, argv):
    import torch
    import torch.distributed as dist
    multi = torch.cuda.device_count() >= world
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank if multi else 0),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    from nbdt import dist as nd
    nd.init_from_env(backend="nccl" if multi else "gloo")       # main() finds the group initialised and uses it
    spec = importlib.util.spec_from_file_location("nbdt_main", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    seen = {}
    step = M.train_step

    def spy(engine, *args, **kwargs):
        seen["engine"] = engine
        return step(engine, *args, **kwargs)
    M.train_step = spy
    acc, nbdt_acc = M.main(argv)
    torch.cuda.synchronize()
    with open(prefix + ".json", "w") as f:
        json.dump({"acc": acc, "nbdt_acc": nbdt_acc}, f)
    if "engine" in seen:
        torch.save(seen["engine"].store.flat.cpu(), prefix + ".pt")
    dist.destroy_process_group()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5:])
