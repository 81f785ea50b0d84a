"""A lexicon for the seq2seq decoder's beam search (include/slu_hip.h, slu_beam_select_lex; DESIGN.md section 7
"Lexicon-constrained search"): a non-empty set of label sequences over [0, V), each ending in eos with eos nowhere else,
compiled into a trie in CSR form.

    trie_off (N + 1)  offsets of each node's edges
    trie_lab (N - 1)  edge labels, ascending within a node
    trie_dst (N - 1)  the child node of each edge

Node 0 is the root; a node is a leaf exactly when its incoming edge is eos.  Nodes are numbered breadth-first with
children in label order, so equal lexicons give equal tables.  No torch until the tables go to a device."""


class Lexicon:
    def __init__(self, sequences, V, eos):
        """sequences: an iterable of label sequences; V: the number of labels; eos: the label that ends every sequence.
        ValueError("lexicon: ...") for an empty set, a label outside [0, V), eos inside a sequence, a missing final eos.
        Duplicates are merged."""
        V, eos = int(V), int(eos)
        if not 0 <= eos < V:
            raise ValueError("lexicon: eos = %r outside [0, %d)" % (eos, V))
        entries = set()
        for seq in sequences:
            seq = tuple(int(c) for c in seq)
            for c in seq:
                if not 0 <= c < V:
                    raise ValueError("lexicon: label %d outside [0, %d) in %r" % (c, V, list(seq)))
            if not seq or seq[-1] != eos:
                raise ValueError("lexicon: missing final eos (%d) in %r" % (eos, list(seq)))
            if eos in seq[:-1]:
                raise ValueError("lexicon: eos (%d) inside a sequence, %r" % (eos, list(seq)))
            entries.add(seq)
        if not entries:
            raise ValueError("lexicon: empty set")
        self.V, self.eos = V, eos
        self.entries = tuple(sorted(entries))
        self.max_len = max(len(e) for e in self.entries)
        # breadth-first over the groups of entries that share a prefix: a node is (its entries, its depth); the entries
        # are sorted, so a node's children come out in label order
        off, lab, dst = [0], [], []
        queue, n_nodes, head = [(self.entries, 0)], 1, 0
        while head < len(queue):
            group, depth = queue[head]
            head += 1
            children = {}
            for e in group:
                if len(e) > depth:
                    children.setdefault(e[depth], []).append(e)
            for c in sorted(children):
                lab.append(c)
                dst.append(n_nodes)
                n_nodes += 1
                queue.append((tuple(children[c]), depth + 1))
            off.append(len(lab))
        self.trie_off, self.trie_lab, self.trie_dst = tuple(off), tuple(lab), tuple(dst)
        self.N = n_nodes
        self._device = {}
        self._levels = None

    @classmethod
    def from_strings(cls, strings, Sy):
        """strings over the label list Sy -> the lexicon of [<sos>] + characters + [<eos>], what data.py builds as y_intent
        for a seq2seq model."""
        index = {c: i for i, c in enumerate(Sy)}
        if "<sos>" not in index or "<eos>" not in index:
            raise ValueError("lexicon: the label list has no <sos> / <eos>")
        seqs = []
        for s in strings:
            for c in s:
                if c not in index:
                    raise ValueError("lexicon: character %r of %r is no label (outside [0, %d))" % (c, s, len(Sy)))
            seqs.append([index["<sos>"]] + [index[c] for c in s] + [index["<eos>"]])
        return cls(seqs, len(Sy), index["<eos>"])

    def __len__(self):
        return len(self.entries)

    def key(self):
        """The lexicon's identity for a search plan: equal lexicons give equal tables, so the tables are the identity."""
        return (self.V, self.eos, self.trie_off, self.trie_lab, self.trie_dst)

    def tables(self, device):
        """(trie_off, trie_lab, trie_dst) int32 tensors on `device`, copied once per device."""
        import torch
        k = str(device)
        if k not in self._device:
            self._device[k] = tuple(torch.tensor(t, dtype=torch.int32).to(device)
                                    for t in (self.trie_off, self.trie_lab, self.trie_dst))
        return self._device[k]

    def levels(self):
        """What the exact sweep over the lexicon needs (include/slu_hip.h, slu_trie_expand), as tuples:

            level_off (max_len + 2)  the nodes of depth d are level_off[d] .. level_off[d + 1] - 1 (breadth-first numbers:
                                     a depth is a contiguous range; depth 0 is the root, depth max_len the last leaves)
            inner (max_len + 1)      per depth, the ascending tuple of its inner nodes (a node is a leaf exactly when its
                                     incoming edge is eos); len(inner[d]) is n_inner[d]
            slot (N)                 an inner node: its index in its depth's inner tuple; a leaf: the index in `entries` of
                                     the entry it ends (entries are sorted; leaves and entries are in bijection)
            width                    max(n_inner)

        -> (level_off, inner, slot, width).  Equal lexicons give equal tables."""
        if self._levels is None:
            depth, leaf, path = [0] * self.N, [False] * self.N, [()] * self.N
            for n in range(self.N):                      # a child's number is larger than its parent's
                for e in range(self.trie_off[n], self.trie_off[n + 1]):
                    c = self.trie_dst[e]
                    depth[c], leaf[c], path[c] = depth[n] + 1, self.trie_lab[e] == self.eos, path[n] + (self.trie_lab[e],)
            level_off = [0] * (self.max_len + 2)
            for d in depth:
                level_off[d + 1] += 1
            for d in range(self.max_len + 1):
                level_off[d + 1] += level_off[d]
            inner = tuple(tuple(n for n in range(level_off[d], level_off[d + 1]) if not leaf[n])
                          for d in range(self.max_len + 1))
            index = {e: i for i, e in enumerate(self.entries)}
            slot = [0] * self.N
            for nodes in inner:
                for i, n in enumerate(nodes):
                    slot[n] = i
            for n in range(self.N):
                if leaf[n]:
                    slot[n] = index[path[n]]
            self._levels = (tuple(level_off), inner, tuple(slot), max(len(nodes) for nodes in inner))
        return self._levels

    @property
    def width(self):
        """The widest level of the sweep: the most inner nodes any depth has."""
        return self.levels()[3]

    def level_tables(self, device):
        """(slot (N) int32, [inner nodes of depth d (n_inner[d]) int32 or None, d = 0 .. max_len]) on `device`, copied once
        per device."""
        import torch
        k = "levels:" + str(device)
        if k not in self._device:
            _, inner, slot, _ = self.levels()
            self._device[k] = (torch.tensor(slot, dtype=torch.int32).to(device),
                               [torch.tensor(nodes, dtype=torch.int32).to(device) if nodes else None for nodes in inner])
        return self._device[k]

    def entry_table(self, device, U):
        """(M, U) int64 on `device`: row m is entry m's labels and then eos to the end (U >= max_len), copied once per device
        and U."""
        import torch
        k = "entries:%d:%s" % (U, device)
        if k not in self._device:
            assert U >= self.max_len
            self._device[k] = torch.tensor([list(e) + [self.eos] * (U - len(e)) for e in self.entries],
                                           dtype=torch.int64).to(device)
        return self._device[k]
