"""NumPy / Python restatement of the reference's test stage, `model_tester.test_model` (/root/reference/model_tester.py:51-170) with its
`process` (:173-237), over in-memory samples and given score vectors instead of files and a TensorFlow model.  Kept close to the
reference's text: Python's `sorted(..., reverse=True)` rankings, the rng consumption of :84-85 and :128-129, NumPy scalar arithmetic
of :199 and :234, and the `csv.DictWriter` / `np.save` outputs of :155-164.  The helper of tests/test_tester_restate.py (hand-worked
cases) and tests/test_gpu_tester.py (the device driver against it)."""
from __future__ import annotations

import csv
import os

import numpy as np


def deviation(pred, true) -> int:
    """First position where the stable descending rankings of `pred` and `true` differ; len(true) when they agree
    (model_tester.py:124-135, 142-147, 211-220)."""
    pred_ranking = np.array(sorted(range(len(pred)), key=lambda x: pred[x], reverse=True))
    true_ranking = np.array(sorted(range(len(true)), key=lambda x: true[x], reverse=True))
    differences = (pred_ranking != true_ranking)
    if np.any(differences):
        return int(np.argmax(pred_ranking != true_ranking))
    return len(true)


def random_deviation(random_ranking, true) -> int:
    true_ranking = np.array(sorted(range(len(true)), key=lambda x: true[x], reverse=True))
    differences = (random_ranking != true_ranking)
    if np.any(differences):
        return int(np.argmax(random_ranking != true_ranking))
    return len(true)


def hybrid_pred(sample_cut):
    """model_tester.py:113-120, in the sample's own dtype."""
    cut_feats = sample_cut['values']
    cut_feat_names = sample_cut['features']
    int_support = cut_feats[:, cut_feat_names.index('int_support')]
    efficacy = cut_feats[:, cut_feat_names.index('efficacy')]
    parallelism = cut_feats[:, cut_feat_names.index('parallelism')]
    return efficacy + 0.1 * int_support + 0.1 * parallelism


def process(samples, predictions, mses, test_batch_size=4):
    """model_tester.process (:173-237) on consecutive batches of `samples`: predictions[b] is the model's fp32 output on batch b (all
    its cuts, in order), mses[b] the batch's fp32 mean squared error.  Improvements are what load_batch_tf gives: fp32."""
    loss = 0
    mean_acc = 0
    n_samples = 0
    cut_count = 0
    for b, start in enumerate(range(0, len(samples), test_batch_size)):
        batch = samples[start:start + test_batch_size]
        n_cuts = np.array([s[0][3]['values'].shape[0] for s in batch], np.int32)
        n_cuts_total = n_cuts.sum(dtype=np.int32)
        batch_size = len(n_cuts)
        loss += n_cuts_total * np.float32(mses[b])
        predictions_b = np.split(np.asarray(predictions[b], np.float32), np.cumsum(n_cuts)[:-1])
        improvements_b = [np.asarray(s[1]).astype(np.float32) for s in batch]
        acc = 0
        for i in range(batch_size):
            pred = predictions_b[i]
            true = improvements_b[i]
            frac = deviation(pred, true) / len(pred)
            acc += frac
        mean_acc += acc
        n_samples += batch_size
        cut_count += n_cuts_total
    loss /= cut_count
    mean_acc /= n_samples
    return loss, mean_acc


def baselines(samples, seed):
    """The random and hybrid baselines (:84-85, :100-153): (random_acc, hybrid_acc) over the file improvements (fp64 on disk)."""
    rng = np.random.default_rng(seed)
    int(rng.integers(np.iinfo(int).max))   # tf.random.set_seed's draw
    random_acc = 0
    hybrid_acc = 0
    for sample in samples:
        sample_state, sample_improvements = sample
        pred = hybrid_pred(sample_state[3])
        true = sample_improvements
        random_ranking = np.arange(len(true))
        rng.shuffle(random_ranking)
        random_acc += random_deviation(random_ranking, true) / len(true)
        hybrid_acc += deviation(pred, true) / len(true)
    random_acc /= len(samples)
    hybrid_acc /= len(samples)
    return random_acc, hybrid_acc


def test_model(samples, predictions, mses, seed, test_batch_size=4):
    """{'loss', 'gcnn', 'hybrid', 'random'} as model_tester.test_model computes them."""
    test_loss, test_acc = process(samples, predictions, mses, test_batch_size)
    random_acc, hybrid_acc = baselines(samples, seed)
    return {'loss': test_loss, 'gcnn': test_acc, 'hybrid': hybrid_acc, 'random': random_acc}


test_model.__test__ = False   # not a pytest test


def write(folder, seed, result):
    """model_tester.py:155-164 into `folder`."""
    os.makedirs(folder, exist_ok=True)
    fieldnames = ['type', 'seed', 'fraction']
    with open(os.path.join(folder, f"{seed}.csv"), 'w', newline='') as csvfile:
        writer = csv.DictWriter(csvfile, fieldnames=fieldnames)
        writer.writeheader()
        writer.writerow({'type': 'random', 'seed': seed, 'fraction': result['random']})
        writer.writerow({'type': 'hybrid', 'seed': seed, 'fraction': result['hybrid']})
        writer.writerow({'type': 'gcnn', 'seed': seed, 'fraction': result['gcnn']})
    np.save(os.path.join(folder, f"{seed}_loss"), np.array(result['loss']))
