"""A worker process of tests/test_gpu_lpmodels.py: tests/serve_worker_lp.py as it is -- NumPy only, opens no GPU, the same requests
and the same checks -- under a model key of its own instead of "m".

usage: serve_worker_lpmodels.py ROOT ADDRESS WORKER_ID OUT.npz READY_FILE MODEL_KEY"""
import sys


def main():
    root, key = sys.argv[1], sys.argv.pop(6)
    sys.path.insert(0, root)
    import serve_worker_lp                                  # (this file's directory is the first entry of sys.path)
    from gcnn_cut_selector_amd import serve
    plain = serve.ScoringClient
    serve.ScoringClient = lambda address, _key, **options: plain(address, key, **options)
    serve_worker_lp.main()


if __name__ == "__main__":
    main()
