'use strict'
/**
 * GpuEngine -- Promise API over the N-API addon (addon/ygm_napi.c -> libygm.so).
 *
 * Requests from many documents that arrive within `batchWindowMs` (or until
 * `maxBatchDocs`) are packed into ONE GPU batch: the batch formation point is
 * the debounced store of Hocuspocus (packages/server/src/Hocuspocus.ts:417-447,
 * SURVEY.md §8a row a4).  One batch is in flight per engine; later requests
 * queue for the next batch.  A document whose status is not OK rejects only its
 * own promise, with yjs's error text (SURVEY.md §8b "Errors").
 */
const path = require('path')
const { jobUpdates } = require('./log')
const now = () => Number(process.hrtime.bigint()) / 1e6

let addon = null
function loadAddon () {
  if (!addon) addon = require(path.join(__dirname, '..', 'build', 'ygm_napi.node'))
  return addon
}

const STATUS = ['OK', 'EMALFORMED', 'ERANGE', 'ENONCANON', 'ESURROGATE', 'EDEPTH', 'ENOMEM', 'EDEVICE', 'EINVAL', 'EUNSUPPORTED']

class YgmError extends Error {
  constructor (code, message) {
    super(message)
    this.name = 'YgmError'
    this.code = STATUS[code] || String(code)
    this.status = code
  }
}

class Batcher {
  constructor (engine, op) {
    this.engine = engine
    this.op = op
    this.queue = []
    this.timer = null
    this.inflight = false
  }

  push (job) {
    return new Promise((resolve, reject) => {
      if (this.queue.length === 0) this.t_first = now()
      this.queue.push({ job, resolve, reject })
      if (this.queue.length >= this.engine.maxBatchDocs) this.kick(0)
      else this.kick(this.engine.batchWindowMs)
    })
  }

  kick (delay) {
    if (this.inflight) return
    if (delay === 0) { if (this.timer) { clearTimeout(this.timer); this.timer = null } setImmediate(() => this.flush()); return }
    if (!this.timer) this.timer = setTimeout(() => { this.timer = null; this.flush() }, delay)
  }

  async flush () {
    if (this.inflight || this.queue.length === 0) return
    const batch = this.queue.splice(0, this.engine.maxBatchDocs)
    this.inflight = true
    const t0 = now()
    try {
      const res = await this.engine._run(this.op, batch.map(b => b.job))
      const t1 = now()
      batch.forEach((b, i) => {
        const st = res.status[i]
        if (st === 0) b.resolve(res.outputs[i])
        else b.reject(new YgmError(st, loadAddon().strerror(st)))
      })
      // the last batch's time split (engine.timing[op]): window wait, JS packing, the native call (worker
      // execution + copy-out), settling the documents' promises
      this.engine.timing[this.op] = { docs: batch.length, wait_ms: t0 - (this.t_first || t0), ...this.engine._last, settle_ms: now() - t1 }
    } catch (e) {
      batch.forEach(b => b.reject(e))
    } finally {
      this.inflight = false
      if (this.queue.length) this.kick(this.queue.length >= this.engine.maxBatchDocs ? 0 : this.engine.batchWindowMs)
    }
  }
}

// one batch arena from merge jobs: an array of updates, or { head: Uint8Array[], arena, lens } whose log part is
// already packed (UpdateLog): one copy per document, and the per-update lengths / document ids by typed-array
// fills instead of per-update pushes
function packJobs (jobs) {
  let nUpd = 0; let total = 0
  for (const j of jobs) {
    if (Array.isArray(j)) { nUpd += j.length; for (const u of j) total += u.length } else {
      nUpd += j.head.length + j.lens.length; total += j.arena.length
      for (const u of j.head) total += u.length
    }
  }
  const arena = Buffer.allocUnsafe(total)
  const lens = new Uint32Array(nUpd)
  const docs = new Uint32Array(nUpd)
  let o = 0; let k = 0
  jobs.forEach((j, d) => {
    const k0 = k
    const ups = Array.isArray(j) ? j : j.head
    for (const u of ups) { arena.set(u, o); o += u.length; lens[k++] = u.length }
    if (!Array.isArray(j)) { arena.set(j.arena, o); o += j.arena.length; lens.set(j.lens, k); k += j.lens.length }
    docs.fill(d, k0, k)
  })
  return { arena, lens, docs }
}

function packBlobs (blobs) {
  const lens = new Uint32Array(blobs.length)
  let total = 0
  for (let i = 0; i < blobs.length; i++) { lens[i] = blobs[i].length; total += blobs[i].length }
  const arena = Buffer.allocUnsafe(total)
  let o = 0
  for (const b of blobs) { arena.set(b, o); o += b.length }
  return { arena, lens }
}

/** YGM_DOC_NO_GC: the option byte of a document created with gc: false (yDocOptions, Hocuspocus.ts:331-344) */
const DOC_NO_GC = 1
/** YGM_TEXT_FLAT / YGM_TEXT_DEEP: the modes of ygm_text_v1 */
const TEXT_FLAT = 0; const TEXT_DEEP = 1
/** YGM_JSON_PROSEMIRROR: the one kind of ygm_json_v1 */
const JSON_PROSEMIRROR = 0
/** YGM_TOJSON_MAP / YGM_TOJSON_ARRAY / YGM_TOJSON_TEXT: the kinds of ygm_tojson_v1 */
const TOJSON_MAP = 0; const TOJSON_ARRAY = 1; const TOJSON_TEXT = 2
/**
 * A document's field list for ygm_json_fields_v1: null, undefined or [] give no bytes (every key of doc.share); names
 * (strings or UTF-8 bytes) give their lib0 varStrings back to back -- a varuint byte length, then the bytes.
 */
function encodeFields (fields) {
  if (fields === null || fields === undefined || fields.length === 0) return Buffer.alloc(0)
  if (!Array.isArray(fields)) throw new YgmError(8, 'a field list is null or an array of names')
  const parts = []
  for (const f of fields) {
    const b = f instanceof Uint8Array ? f : Buffer.from(String(f), 'utf8')
    const head = []
    let n = b.length
    while (n > 127) { head.push(0x80 | (n & 127)); n >>>= 7 }
    head.push(n)
    parts.push(Buffer.from(head), b)
  }
  return Buffer.concat(parts)
}
// per-document options -> option bytes, or undefined when none is set (the plain native entry points): an entry is an
// option byte, `true` (no-GC), or { gc: boolean } as in yDocOptions; a Uint8Array is taken as it is
function optBytes (opts, n) {
  if (opts === undefined || opts === null) return undefined
  if (opts.length !== n) throw new YgmError(8, 'one option per document')
  const out = opts instanceof Uint8Array ? opts : Uint8Array.from(opts, o => typeof o === 'number' ? o : o === true ? DOC_NO_GC : o && o.gc === false ? DOC_NO_GC : 0)
  return out.some(b => b !== 0) ? out : undefined
}

// ---- the batched ops of GpuEngine._run: `native` is the addon function (a row of OPS[] in addon/ygm_napi.c), `pack`
// turns the jobs into its arena arguments, `extra` gives its trailing argument, `timed` keeps the time split (_last)
const arenas = (...blobLists) => blobLists.flatMap(blobs => { const p = packBlobs(blobs); return [p.arena, p.lens] })
const packMerge = jobs => { const { arena, lens, docs } = packJobs(jobs); return [arena, lens, docs] }
const packOne = jobs => arenas(jobs)                                           // a job is an update / a state
const packPair = jobs => arenas(jobs.map(j => j[0]), jobs.map(j => j[1]))      // a job is [first, second(, option byte)]
const pairOpts = jobs => optBytes(jobs.map(j => j[2] || 0), jobs.length)
const OPS = {
  merge: { native: 'mergeMany', pack: packMerge, extra: jobs => jobs.length, timed: true },
  mergeV2: { native: 'mergeManyV2', pack: packMerge, extra: jobs => jobs.length, timed: true },
  diff: { native: 'diffMany', pack: packPair },
  diffV2: { native: 'diffManyV2', pack: packPair },
  contains: { native: 'containsMany', pack: packPair },
  step2: { native: 'step2Many', pack: packPair, extra: pairOpts },
  restoreVersion: { native: 'restoreVersionMany', pack: packPair, extra: pairOpts },
  text: { native: 'text', pack: packPair, extra: () => TEXT_FLAT },             // a job is [state, root name bytes]
  textDeep: { native: 'text', pack: packPair, extra: () => TEXT_DEEP },
  json: { native: 'json', pack: packPair, extra: () => JSON_PROSEMIRROR },
  jsonFields: { native: 'jsonFields', pack: packPair, extra: () => JSON_PROSEMIRROR },   // a job is [state, encoded field list]
  toJson: { native: 'toJson', pack: packPair, extra: jobs => jobs.length ? jobs[0][2] : TOJSON_MAP },   // a job is [state, root name bytes, the batch's kind]
  // a job is an update, or { update, opt } for one with an option byte: both kinds share a window
  snapshot: { native: 'snapshotMany', pack: jobs => arenas(jobs.map(j => j instanceof Uint8Array ? j : j.update)),
    extra: jobs => optBytes(jobs.map(j => j instanceof Uint8Array ? 0 : j.opt), jobs.length) },
  takeVersion: { native: 'takeVersionMany', pack: packOne },
  sv: { native: 'svMany', pack: packOne },
  svV2: { native: 'svManyV2', pack: packOne },
  v1ToV2: { native: 'convertManyV1ToV2', pack: packOne },
  v2ToV1: { native: 'convertManyV2ToV1', pack: packOne }
}

class GpuEngine {
  /**
   * @param {{device?: number, compat135?: boolean, floats?: boolean, batchWindowMs?: number, maxBatchDocs?: number}} [opts]
   *   floats (YGM_F_FLOATS, off by default): jsonMany / jsonFieldsMany / toJsonMany write non-integer numbers as
   *   JSON.stringify does, where they refuse the document (ENONCANON) without it
   */
  constructor (opts = {}) {
    this.device = opts.device || 0
    this.flags = (opts.compat135 ? 1 : 0) | (opts.floats ? 8 : 0)
    this.batchWindowMs = opts.batchWindowMs === undefined ? 2 : opts.batchWindowMs
    this.maxBatchDocs = opts.maxBatchDocs || 65536
    this.handle = loadAddon().open(this.device, this.flags)
    this.batchers = { merge: new Batcher(this, 'merge'), diff: new Batcher(this, 'diff'), sv: new Batcher(this, 'sv'), snapshot: new Batcher(this, 'snapshot'),
      takeVersion: new Batcher(this, 'takeVersion'), restoreVersion: new Batcher(this, 'restoreVersion') }
    this.timing = {}
    this._last = {}
    this.chain = Promise.resolve()
  }

  // one native batch at a time per handle (the addon enforces it; chain them here)
  _chain (run) {
    const p = this.chain.then(run, run)
    this.chain = p.catch(() => {})
    return p
  }

  // one batch of `op` (a row of OPS): pack the jobs, call the row's addon function with the row's trailing value
  _run (op, jobs) {
    const { native, pack, extra, timed } = OPS[op]
    return this._chain(() => {
      const t0 = now()
      const args = pack(jobs)
      const t1 = now()
      if (extra) args.push(extra(jobs))
      if (!timed) return loadAddon()[native](this.handle, ...args)
      const s0 = this.stats()
      const p = loadAddon()[native](this.handle, ...args)
      const t2 = now()
      return p.then(r => {
        const s1 = this.stats()
        this._last = { pack_ms: t1 - t0, napi_in_ms: t2 - t1, native_ms: now() - t2, exec_ms: r.execMs, copy_out_ms: r.completeMs,
          h2d_ms: s1.h2dMs - s0.h2dMs, kernel_ms: s1.kernelMs - s0.kernelMs, d2h_ms: s1.d2hMs - s0.d2hMs, bytes: args[0].length }
        return r
      })
    })
  }

  /** Y.mergeUpdates(updates), batched with concurrent callers. */
  mergeUpdates (updates) { return this.batchers.merge.push(updates.map(u => u instanceof Uint8Array ? u : Uint8Array.from(u))) }
  /** Y.mergeUpdates([...head, ...the packed updates]) for { head: Uint8Array[], arena, lens } (UpdateLog.packed) */
  mergePacked (job) { return this.batchers.merge.push(job) }
  /** Y.diffUpdate(update, stateVector) */
  diffUpdate (update, sv) { return this.batchers.diff.push([update, sv]) }
  /** Y.encodeStateVectorFromUpdate(update) */
  encodeStateVectorFromUpdate (update) { return this.batchers.sv.push(update) }
  /** Y.encodeStateAsUpdate(Y.applyUpdate(new Y.Doc(), update)): the doc-normalized snapshot (GC'd, merged);
   *  { gc: false }: of new Y.Doc({ gc: false }) -- deleted content kept, as a document created with that option stores it */
  snapshot (update, { gc } = {}) {
    const u = update instanceof Uint8Array ? update : Uint8Array.from(update)
    return this.batchers.snapshot.push(gc === false ? { update: u, opt: DOC_NO_GC } : u)
  }

  /** explicit batches (sync responders, bulk snapshot jobs) */
  async mergeMany (docs) { const r = await this._run('merge', docs); return unpack(r) }
  async diffMany (states, svs) { const r = await this._run('diff', states.map((s, i) => [s, svs[i]])); return unpack(r) }
  /** SyncStep2 payloads of stored documents: Y.encodeStateAsUpdate(doc, sv) of doc = Y.applyUpdate(new Y.Doc(), state)
   *  (MessageReceiver.ts:137-138) -- the snapshot, then a diff keeping each struct's parentSub bit; EUNSUPPORTED
   *  outside the snapshot envelope */
  async step2Many (states, svs, opts) {
    const o = optBytes(opts, states.length)
    const r = await this._run('step2', states.map((s, i) => [s, svs[i], o ? o[i] : 0]))
    return unpack(r)
  }
  /**
   * Many state vectors answered from shared states (a reconnect storm): ask a is answered from states[askState[a]]
   * with svs[a].  diffShared: Y.diffUpdate per ask; step2Shared: the SyncStep2 payload per ask, byte for byte what
   * step2Many gives for the pair -- but every state is uploaded and snapshotted once, however many asks name it.
   * The asks are sorted by state here (the native call takes them non-decreasing); results come back in caller order.
   * step2Shared's opts: one option per state (as snapshotMany's), which all of the state's asks are answered with.
   */
  diffShared (states, askState, svs) { return this._shared('diffShared', states, askState, svs) }
  step2Shared (states, askState, svs, opts) { return this._shared('step2Shared', states, askState, svs, optBytes(opts, states.length)) }
  /**
   * Many versions restored from shared states (a history sidebar, a scrubber, an export of every version): ask a restores
   * versions[a] from states[askState[a]], byte for byte what restoreVersionMany gives for the pair -- but every state
   * is uploaded and given its no-GC snapshot once, however many versions name it.  opts: one option per ask (as
   * restoreVersionMany's, one per pair): the option belongs to the restored document, not to the state.
   */
  restoreVersionShared (states, askState, versions, opts) {
    return this._shared('restoreVersionShared', states, askState, versions, optBytes(opts, versions.length), true)
  }

  async _shared (op, states, askState, svs, opt, optPerAsk) {
    const n = svs.length
    if (askState.length !== n) throw new YgmError(8, 'one state index per state vector')
    for (let a = 0; a < n; a++) {
      if (!Number.isInteger(askState[a]) || askState[a] < 0 || askState[a] >= states.length) throw new YgmError(8, loadAddon().strerror(8))
    }
    const order = Array.from({ length: n }, (_, a) => a).sort((x, y) => askState[x] - askState[y] || x - y)
    const r = unpack(await this._chain(() => {
      const o = opt && optPerAsk ? Uint8Array.from(order, a => opt[a]) : opt   // (per-ask bytes travel with their asks)
      return loadAddon()[op](this.handle, ...arenas(states, order.map(a => svs[a])), Uint32Array.from(order, a => askState[a]), o)
    }))
    const out = new Array(n)
    order.forEach((a, k) => { out[a] = r[k] })
    return out
  }

  async stateVectorsMany (states) { const r = await this._run('sv', states); return unpack(r) }
  /** snapshots as an explicit batch; opts: one option per state -- an option byte, true, or { gc: false } for a
   *  document created with gc: false (both kinds in one batch) */
  async snapshotMany (states, opts) {
    const o = optBytes(opts, states.length)
    const r = await this._run('snapshot', o ? states.map((s, i) => ({ update: s, opt: o[i] })) : states)
    return unpack(r)
  }
  /** Y.snapshotContainsUpdate(Y.snapshot(doc), update) per pair, `states` being normalized (snapshotMany) states */
  async containsMany (states, updates) {
    const r = await this._run('contains', states.map((s, i) => [s, updates[i]]))
    return unpack(r).map(x => x instanceof Error ? x : x[0] === 1)
  }

  /**
   * Version history.  takeVersion: Y.encodeSnapshot(Y.snapshot(doc)) of doc = Y.applyUpdate(new Y.Doc(), state);
   * restoreVersion: Y.encodeStateAsUpdate(Y.createDocFromSnapshot(doc, Y.decodeSnapshot(version), newDoc)) of
   * doc = Y.applyUpdate(new Y.Doc({ gc: false }), state), newDoc = new Y.Doc() or, with { gc: false }, new
   * Y.Doc({ gc: false }).  The single forms share a batch with the calls of the same window; the *Many forms are
   * explicit batches (opts as snapshotMany's, one per pair).  To restore several versions of a document use
   * restoreVersionShared: the pair forms stage and snapshot its state once per version (the batched single call keeps
   * the pair form; states are not compared by content).
   */
  takeVersion (state) { return this.batchers.takeVersion.push(state instanceof Uint8Array ? state : Uint8Array.from(state)) }
  restoreVersion (state, version, { gc } = {}) { return this.batchers.restoreVersion.push([state, version, gc === false ? DOC_NO_GC : 0]) }
  async takeVersionMany (states) { const r = await this._run('takeVersion', states); return unpack(r) }
  async restoreVersionMany (states, versions, opts) {
    if (versions.length !== states.length) throw new YgmError(8, 'one version per state')
    const o = optBytes(opts, states.length)
    const r = await this._run('restoreVersion', states.map((s, i) => [s, versions[i], o ? o[i] : 0]))
    return unpack(r)
  }

  /**
   * Plain text of stored documents, as an explicit batch: for doc = Y.applyUpdate(new Y.Doc(), states[i]) the string
   * doc.getText(names[i]).toString(), or with { deep: true } the walk that also descends into nested types -- the text
   * of an XmlFragment / Tiptap document, one '\n' after each nested type unless the text is still empty or already
   * ends in one (ygm_text_v1).  names: strings or UTF-8 bytes.  A name the state has no root for gives ''.
   */
  async textMany (states, names, { deep = false } = {}) {
    return unpackUtf8(await this._run(deep ? 'textDeep' : 'text', rootJobs(states, names)))
  }

  /**
   * Stored documents as ProseMirror / Tiptap JSON, as an explicit batch: for doc = Y.applyUpdate(new Y.Doc(), states[i])
   * the string JSON.stringify(yXmlFragmentToProsemirrorJSON(doc.getXmlFragment(names[i]))) -- what
   * TiptapTransformer.fromYdoc(doc, names[i]) returns, stringified (ygm_json_v1).  names: strings or UTF-8 bytes.  A
   * name the state has no root for gives '{"type":"doc","content":[]}'; a document outside the envelope (a root that
   * is no XmlFragment of elements and texts, a float, ...) gives a YgmError in its place.
   */
  async jsonMany (states, names) {
    return unpackUtf8(await this._run('json', rootJobs(states, names)))
  }

  /**
   * Every asked field of stored documents as one JSON object, as an explicit batch: for
   * doc = Y.applyUpdate(new Y.Doc(), states[i]) the string JSON.stringify(TiptapTransformer.fromYdoc(doc, fields[i]))
   * -- the `document` of a change webhook (ygm_json_fields_v1).  fields[i]: null, undefined or [] for every key of
   * doc.share, or an array of names (strings or UTF-8 bytes).  One load of the state serves all its fields.  Keys
   * follow JavaScript's own-property order; a document with a refusing field, or a field named __proto__, gives a
   * YgmError in its place.
   */
  async jsonFieldsMany (states, fields) {
    if (fields.length !== states.length) throw new YgmError(8, 'one field list per state')
    return unpackUtf8(await this._run('jsonFields', states.map((s, i) => [s, encodeFields(fields[i])])))
  }

  /**
   * toJSON of stored documents' Map, Array or Text roots, as an explicit batch: for doc = Y.applyUpdate(new Y.Doc(),
   * states[i]) the string JSON.stringify(doc.getMap(names[i]).toJSON()) (kind TOJSON_MAP), of getArray (TOJSON_ARRAY)
   * or of getText (TOJSON_TEXT) -- what a custom webhook transformer's fromYdoc returns, stringified (ygm_tojson_v1).
   * One kind per batch.  A name the state has no root for gives '{}', '[]' or '""'; a document outside the envelope (a
   * nested Xml type, binary content, a non-integer number, ...) gives a YgmError in its place.
   */
  async toJsonMany (states, names, kind) {
    if (kind !== TOJSON_MAP && kind !== TOJSON_ARRAY && kind !== TOJSON_TEXT) throw new YgmError(8, loadAddon().strerror(8))
    return unpackUtf8(await this._run('toJson', rootJobs(states, names).map(j => [j[0], j[1], kind])))
  }

  /** update format V2 (yjs providers other than Hocuspocus's V1 path): Y.mergeUpdatesV2 / Y.diffUpdateV2 /
   *  Y.encodeStateVectorFromUpdateV2 / yjs 13.6 Y.convertUpdateFormatV1ToV2 / V2ToV1, as explicit batches */
  async mergeManyV2 (docs) { const r = await this._run('mergeV2', docs); return unpack(r) }
  async diffManyV2 (states, svs) { const r = await this._run('diffV2', states.map((s, i) => [s, svs[i]])); return unpack(r) }
  async stateVectorsManyV2 (states) { const r = await this._run('svV2', states); return unpack(r) }
  async convertManyV1ToV2 (updates) { const r = await this._run('v1ToV2', updates); return unpack(r) }
  async convertManyV2ToV1 (updates) { const r = await this._run('v2ToV1', updates); return unpack(r) }

  stats () { return loadAddon().stats(this.handle) }
  close () { if (this.handle) { loadAddon().close(this.handle); this.handle = null } }
}

function unpack (r) {
  return Array.from(r.status, (st, i) => st === 0 ? r.outputs[i] : new YgmError(st, loadAddon().strerror(st)))
}
// the text / JSON calls: jobs of [state, root name bytes] (names: strings or UTF-8 bytes); each output as a string
function rootJobs (states, names) {
  if (names.length !== states.length) throw new YgmError(8, 'one root name per state')
  return states.map((s, i) => [s, names[i] instanceof Uint8Array ? names[i] : Buffer.from(String(names[i]), 'utf8')])
}
function unpackUtf8 (r) {
  return unpack(r).map(x => x instanceof Error ? x : Buffer.from(x.buffer, x.byteOffset, x.length).toString('utf8'))
}

const FNV_OFFSET = BigInt('0xcbf29ce484222325')
const FNV_PRIME = BigInt('0x100000001b3')
const U64 = BigInt('0xffffffffffffffff')
/** FNV-1a 64 over the UTF-8 bytes of a document name (SURVEY.md §8e: gpu = fnv1a64(name) mod N). */
function fnv1a64 (name) {
  let h = FNV_OFFSET
  for (const b of Buffer.from(String(name), 'utf8')) h = ((h ^ BigInt(b)) * FNV_PRIME) & U64
  return h
}

/**
 * Documents sharded over several GPUs of one node: one GpuEngine (context, stream, batcher) per
 * device, document -> device by fnv1a64(documentName) mod N, no cross-device traffic (documents
 * are independent; the reference scales by document too, docs/guides/scalability.md:12-14).
 * Same API as GpuEngine with a trailing document name; the *Many forms split a batch by shard,
 * run the shards concurrently (one native worker thread per device handle, addon/ygm_napi.c) and return results in caller order.
 */
class GpuEnginePool {
  constructor (opts = {}) {
    const devices = opts.devices && opts.devices.length ? opts.devices : [opts.device || 0]
    const make = opts.makeEngine || (device => new GpuEngine({ ...opts, device }))
    this.engines = devices.map(make)
  }

  shardOf (documentName) { return Number(fnv1a64(documentName) % BigInt(this.engines.length)) }
  engineFor (documentName) { return this.engines[this.shardOf(documentName)] }
  mergeUpdates (updates, documentName = '') { return this.engineFor(documentName).mergeUpdates(updates) }
  mergePacked (job, documentName = '') {
    const e = this.engineFor(documentName)
    return e.mergePacked ? e.mergePacked(job) : e.mergeUpdates(jobUpdates(job))
  }
  diffUpdate (update, sv, documentName = '') { return this.engineFor(documentName).diffUpdate(update, sv) }
  encodeStateVectorFromUpdate (update, documentName = '') { return this.engineFor(documentName).encodeStateVectorFromUpdate(update) }
  snapshot (update, documentName = '', opts) { return this.engineFor(documentName).snapshot(update, opts) }

  async _many (names, cols, run) {
    const parts = this.engines.map(() => [])
    names.forEach((n, i) => parts[this.shardOf(n)].push(i))
    const out = new Array(names.length)
    await Promise.all(parts.map(async (idx, e) => {
      if (!idx.length) return
      const r = await run(this.engines[e], ...cols.map(c => idx.map(i => c[i])))
      idx.forEach((i, k) => { out[i] = r[k] })
    }))
    return out
  }

  mergeMany (names, docs) { return this._many(names, [docs], (e, d) => e.mergeMany(d)) }
  diffMany (names, states, svs) { return this._many(names, [states, svs], (e, a, b) => e.diffMany(a, b)) }
  step2Many (names, states, svs, opts) {
    if (!opts) return this._many(names, [states, svs], (e, a, b) => e.step2Many(a, b))
    return this._many(names, [states, svs, Array.from(opts)], (e, a, b, o) => e.step2Many(a, b, o))
  }
  /**
   * The shared-state forms with one name per state: states go to their fnv1a64(name) shard, each shard's asks are
   * re-indexed to its own states, the shards run concurrently and the results return in caller (ask) order.
   */
  diffShared (names, states, askState, svs) { return this._sharedMany('diffShared', names, states, askState, svs) }
  step2Shared (names, states, askState, svs, opts) { return this._sharedMany('step2Shared', names, states, askState, svs, opts) }
  /** restoreVersionShared with one name per state; opts: one option per ask, routed with its ask */
  restoreVersionShared (names, states, askState, versions, opts) { return this._sharedMany('restoreVersionShared', names, states, askState, versions, opts, true) }
  async _sharedMany (op, names, states, askState, svs, opts, optPerAsk) {
    if (opts && opts.length !== (optPerAsk ? svs.length : states.length)) throw new YgmError(8, optPerAsk ? 'one option per ask' : 'one option per state')
    if (names.length !== states.length || askState.length !== svs.length) throw new YgmError(8, 'one name per state, one state index per state vector')
    const shard = names.map(n => this.shardOf(n))
    const local = new Array(states.length)   // a state's index inside its shard
    const parts = this.engines.map(() => ({ states: [], asks: [], opts: [] }))
    states.forEach((s, i) => { local[i] = parts[shard[i]].states.length; parts[shard[i]].states.push(s); if (opts && !optPerAsk) parts[shard[i]].opts.push(opts[i]) })
    for (let a = 0; a < svs.length; a++) {
      const i = askState[a]
      if (!Number.isInteger(i) || i < 0 || i >= states.length) throw new YgmError(8, 'ask names no state')
      parts[shard[i]].asks.push(a)
      if (opts && optPerAsk) parts[shard[i]].opts.push(opts[a])
    }
    const out = new Array(svs.length)
    await Promise.all(parts.map(async (p, e) => {
      if (!p.asks.length) return
      const r = opts
        ? await this.engines[e][op](p.states, p.asks.map(a => local[askState[a]]), p.asks.map(a => svs[a]), p.opts)
        : await this.engines[e][op](p.states, p.asks.map(a => local[askState[a]]), p.asks.map(a => svs[a]))
      p.asks.forEach((a, k) => { out[a] = r[k] })
    }))
    return out
  }

  stateVectorsMany (names, states) { return this._many(names, [states], (e, a) => e.stateVectorsMany(a)) }
  snapshotMany (names, states, opts) {
    if (!opts) return this._many(names, [states], (e, a) => e.snapshotMany(a))
    return this._many(names, [states, Array.from(opts)], (e, a, o) => e.snapshotMany(a, o))
  }
  containsMany (names, states, updates) { return this._many(names, [states, updates], (e, a, b) => e.containsMany(a, b)) }
  takeVersionMany (names, states) { return this._many(names, [states], (e, a) => e.takeVersionMany(a)) }
  restoreVersionMany (names, states, versions, opts) {
    if (!opts) return this._many(names, [states, versions], (e, a, b) => e.restoreVersionMany(a, b))
    return this._many(names, [states, versions, Array.from(opts)], (e, a, b, o) => e.restoreVersionMany(a, b, o))
  }
  /** textMany with one document name per state (the shard), beside its root name */
  textMany (docNames, states, names, opts) { return this._many(docNames, [states, names], (e, a, b) => e.textMany(a, b, opts)) }
  /** jsonMany with one document name per state (the shard), beside its root name */
  jsonMany (docNames, states, names) { return this._many(docNames, [states, names], (e, a, b) => e.jsonMany(a, b)) }
  /** jsonFieldsMany with one document name per state (the shard), beside its field list */
  jsonFieldsMany (docNames, states, fields) { return this._many(docNames, [states, fields], (e, a, b) => e.jsonFieldsMany(a, b)) }
  /** toJsonMany with one document name per state (the shard), beside its root name */
  toJsonMany (docNames, states, names, kind) { return this._many(docNames, [states, names], (e, a, b) => e.toJsonMany(a, b, kind)) }
  stats () { return this.engines.map(e => e.stats()) }
  /**
   * Node-wide totals (the reference's server-wide counters, Hocuspocus.ts:138-160): every numeric field of the
   * per-device stats summed over the pool's engines, plus `devices`.  Read on the host from each context's counters:
   * no collective, nothing crosses GPUs.
   */
  statsTotal () {
    const t = { devices: this.engines.length }
    for (const s of this.stats()) for (const [k, v] of Object.entries(s)) if (typeof v === 'number') t[k] = (t[k] || 0) + v
    return t
  }
  close () { this.engines.forEach(e => e.close()) }
}

module.exports = { packJobs, GpuEngine, GpuEnginePool, fnv1a64, YgmError, STATUS, loadAddon, DOC_NO_GC, TEXT_FLAT, TEXT_DEEP, TOJSON_MAP, TOJSON_ARRAY, TOJSON_TEXT, optBytes, encodeFields }
