'use strict'
// Documents created with gc: false through the extension: node test/gc.js --cpu|--gpu
//  --cpu : GpuMerge / SyncResponder over an engine double built from the bundled yjs (snapshot of an update into
//          new Y.Doc({ gc }), encodeStateAsUpdate(doc, sv) of that document); checks what the extension asks of the engine
//  --gpu : the same through the N-API addon (compat135: the bundle is yjs 13.5.16), byte for byte against yjs
// The reference builds a document with yDocOptions { gc } (types.ts:152-154, Hocuspocus.ts:331-344, Document.ts:48-49) and
// extension-database stores Y.encodeStateAsUpdate of it (Database.ts:55-60): deleted content survives a store.
const path = require('path')
const assert = require('assert')
const { GpuMerge, DocumentStore, SyncResponder } = require('../src/index.js')
const { frame, MessageType, SyncStep } = require('../src/sync.js')

const mode = process.argv.includes('--gpu') ? 'gpu' : 'cpu'
const Y = require(path.join(__dirname, '..', '..', '..', 'tools', 'yjs_bundle.js')).load()   // the test oracle: yjs from the image's bundle

const hex = b => Buffer.from(b).toString('hex')
const load = (state, gc) => { const d = new Y.Doc({ gc }); Y.applyUpdate(d, state); return d }
const snapshotOf = (state, gc) => Y.encodeStateAsUpdate(load(state, gc))
const isNoGc = o => o === 1 || o === true || !!(o && o.gc === false)

// test double (never shipped): the engine calls the extension and the responder make, from yjs
class GcDouble {
  constructor () { this.log = [] }
  async mergeUpdates (updates) { return Y.mergeUpdates(updates) }
  async mergeMany (docs) { return docs.map(u => Y.mergeUpdates(u)) }
  async stateVectorsMany (states) { return states.map(u => Y.encodeStateVectorFromUpdate(u)) }
  async snapshot (update, opts) { this.log.push(['snapshot', opts && opts.gc]); return snapshotOf(update, !(opts && opts.gc === false)) }
  async step2Shared (states, askState, svs, opts) {
    this.log.push(['step2Shared', opts ? Array.from(opts, isNoGc) : null])
    return svs.map((sv, a) => Y.encodeStateAsUpdate(load(states[askState[a]], !(opts && isNoGc(opts[askState[a]]))), sv))
  }
  close () {}
}

class MemoryStore extends DocumentStore {
  constructor () { super(); this.rows = new Map() }
  async fetchMany (payloads) { return payloads.map(p => this.rows.get(p.documentName) || null) }
  async storeMany (entries) { for (const e of entries) this.rows.set(e.payload.documentName, Uint8Array.from(e.state)) }
}

// two clients edit a document (insertions, then deletions of text, of a map entry and of a nested type); `before` is a
// Y.snapshot taken before the deletions
function edit (doc) {
  const peer = new Y.Doc({ gc: false })
  peer.clientID = 77
  doc.getText('t').insert(0, 'hello brave new world')
  doc.getMap('m').set('k', 'first')
  const nested = new Y.Array()
  doc.getArray('a').insert(0, [nested, 'x'])
  nested.push(['n1', 'n2'])
  Y.applyUpdate(peer, Y.encodeStateAsUpdate(doc))
  peer.getText('t').insert(5, ' there,')
  Y.applyUpdate(doc, Y.encodeStateAsUpdate(peer, Y.encodeStateVector(doc)), 'remote')
  const before = Y.encodeSnapshot(Y.snapshot(doc))
  const textBefore = doc.getText('t').toString()
  doc.getText('t').delete(3, 12)
  doc.getMap('m').set('k', 'second')
  doc.getArray('a').delete(0, 1)
  return { before, textBefore }
}

async function openDoc (ext, name, gc) {
  const document = new Y.Doc({ gc })
  document.clientID = gc ? 11 : 12
  document.name = name
  const payload = { document, documentName: name, context: {}, requestParameters: new Map() }
  await ext.onLoadDocument(payload)
  await ext.afterLoadDocument(payload)
  return payload
}

function makeEngine () {
  if (mode === 'cpu') return new GcDouble()
  const { GpuEngine } = require('../src/engine.js')
  return new GpuEngine({ device: 0, batchWindowMs: 5, compat135: true })
}

const tests = []
const test = (name, fn) => tests.push({ name, fn })

test('a gc: false document and a collected one, stored in one window, each get yjs\'s bytes', async () => {
  const engine = makeEngine()
  const store = new MemoryStore()
  const ext = new GpuMerge({ engine, store, Y })
  try {
    const keep = await openDoc(ext, 'keep', false)
    const drop = await openDoc(ext, 'drop', true)
    const k = edit(keep.document)
    edit(drop.document)
    await Promise.all([ext.onStoreDocument(keep), ext.onStoreDocument(drop)])   // one batch window
    const keepBytes = store.rows.get('keep'); const dropBytes = store.rows.get('drop')
    // what extension-database stores: encodeStateAsUpdate of the live document, loaded afresh with the same option
    assert.strictEqual(hex(keepBytes), hex(snapshotOf(Y.encodeStateAsUpdate(keep.document), false)))
    assert.strictEqual(hex(dropBytes), hex(snapshotOf(Y.encodeStateAsUpdate(drop.document), true)))
    assert.ok(keepBytes.length > dropBytes.length, 'the uncollected state holds the deleted content')
    assert.notStrictEqual(hex(keepBytes), hex(snapshotOf(Y.encodeStateAsUpdate(keep.document), true)))
    if (mode === 'cpu') assert.deepStrictEqual(engine.log.filter(c => c[0] === 'snapshot').map(c => c[1]).sort(), [false, undefined].sort())

    // the user-visible point: after a reload, a snapshot from before the deletion restores the deleted text
    const reloaded = load(keepBytes, false)
    const restored = Y.createDocFromSnapshot(reloaded, Y.decodeSnapshot(k.before))
    assert.strictEqual(restored.getText('t').toString(), k.textBefore)
    assert.strictEqual(restored.getMap('m').get('k'), 'first')
    assert.strictEqual(reloaded.getText('t').toString(), keep.document.getText('t').toString())

    // SyncStep1 for both documents: encodeStateAsUpdate(doc, sv) of the respective live documents
    const responder = ext.syncResponder()
    const svs = [Uint8Array.from([0]), Y.encodeStateVector((() => { const d = new Y.Doc(); d.clientID = 11; d.getText('t').insert(0, 'hello'); return d })())]
    const asks = [['keep', svs[0]], ['drop', svs[0]], ['keep', svs[1]], ['drop', svs[0]]]
    const out = await responder.answerMany(asks.map(([n, sv]) => frame(n, MessageType.Sync, SyncStep.Step1, sv)), { path: 'none' })
    out.forEach((o, i) => {
      assert.ok(Array.isArray(o), 'message ' + i + ': ' + o)
      const live = asks[i][0] === 'keep' ? keep.document : drop.document
      assert.strictEqual(hex(o[0]), hex(frame(asks[i][0], MessageType.Sync, SyncStep.Step2, Y.encodeStateAsUpdate(live, asks[i][1]))), 'message ' + i)
    })
    assert.deepStrictEqual(responder.unnormalized, [])
    if (mode === 'cpu') assert.deepStrictEqual(engine.log.filter(c => c[0] === 'step2Shared').map(c => c[1].slice().sort()), [[false, true]])
  } finally { engine.close() }
})

test('gc: true / false in the configuration override the documents; a bad value is refused', async () => {
  const engine = makeEngine()
  try {
    for (const gc of [true, false]) {
      const store = new MemoryStore()
      const ext = new GpuMerge({ engine, store, Y, gc })
      const p = await openDoc(ext, 'doc', !gc)   // the document says the opposite
      const ups = []
      p.document.on('update', u => ups.push(u))
      edit(p.document)
      await ext.onStoreDocument(p)
      // forced on: the collected form of the document; forced off: what the captured updates hold, uncollected (the
      // live document has dropped its deleted content, the log has not)
      assert.strictEqual(hex(store.rows.get('doc')), hex(snapshotOf(Y.mergeUpdates(ups), gc)))
      if (gc) assert.strictEqual(hex(store.rows.get('doc')), hex(snapshotOf(Y.encodeStateAsUpdate(p.document), true)))
    }
    assert.throws(() => new GpuMerge({ engine, gc: 'sometimes' }), TypeError)
  } finally { engine.close() }
})

test('a responder without getDocOptions asks as before', async () => {
  const engine = makeEngine()
  try {
    const d = new Y.Doc({ gc: false }); d.clientID = 5
    edit(d)
    const state = Y.encodeStateAsUpdate(d)
    const r = new SyncResponder({ engine, getState: async () => state })
    const out = await r.answerMany([frame('x', MessageType.Sync, SyncStep.Step1, Uint8Array.from([0]))], { path: 'none' })
    assert.strictEqual(hex(out[0][0]), hex(frame('x', MessageType.Sync, SyncStep.Step2, snapshotOf(state, true))))
    if (mode === 'cpu') assert.deepStrictEqual(engine.log, [['step2Shared', null]])
    const r2 = new SyncResponder({ engine, getState: async () => state, getDocOptions: () => ({ gc: false }) })
    const out2 = await r2.answerMany([frame('x', MessageType.Sync, SyncStep.Step1, Uint8Array.from([0]))], { path: 'none' })
    assert.strictEqual(hex(out2[0][0]), hex(frame('x', MessageType.Sync, SyncStep.Step2, Y.encodeStateAsUpdate(d))))
  } finally { engine.close() }
})

if (mode === 'gpu') {
  test('the addon: both kinds in one snapshot window and one explicit batch; a bad option byte fails its document only', async () => {
    const engine = makeEngine()
    try {
      const d = new Y.Doc({ gc: false }); d.clientID = 9
      edit(d)
      const u = Y.encodeStateAsUpdate(d)
      const s0 = engine.stats()
      const [a, b, c] = await Promise.all([engine.snapshot(u), engine.snapshot(u, { gc: false }), engine.snapshot(u, { gc: true })])
      assert.strictEqual(engine.stats().calls - s0.calls, 1, 'one batch for the window')
      assert.strictEqual(hex(a), hex(snapshotOf(u, true)))
      assert.strictEqual(hex(b), hex(snapshotOf(u, false)))
      assert.strictEqual(hex(c), hex(a))
      const many = await engine.snapshotMany([u, u, u, u], [0, 1, 2, { gc: false }])
      assert.strictEqual(hex(many[0]), hex(a)); assert.strictEqual(hex(many[1]), hex(b)); assert.strictEqual(hex(many[3]), hex(b))
      assert.ok(many[2] instanceof Error && many[2].code === 'EINVAL')
      const sv = Uint8Array.from([0])
      const pair = await engine.step2Many([u, u], [sv, sv], [{ gc: false }, { gc: true }])
      assert.strictEqual(hex(pair[0]), hex(Y.encodeStateAsUpdate(load(u, false), sv)))
      assert.strictEqual(hex(pair[1]), hex(Y.encodeStateAsUpdate(load(u, true), sv)))
      const shared = await engine.step2Shared([u, u], [1, 0, 1], [sv, sv, sv], [true, false])
      assert.deepStrictEqual(shared.map(hex), [hex(pair[1]), hex(pair[0]), hex(pair[1])])
    } finally { engine.close() }
  })
}

;(async () => {
  let failed = 0
  for (const t of tests) {
    try { await t.fn(); console.log('ok   ' + t.name) } catch (e) { failed++; console.log('FAIL ' + t.name + '\n' + (e && e.stack || e)) }
  }
  console.log(failed ? failed + ' failed' : tests.length + ' passed (' + mode + ')')
  process.exit(failed ? 1 : 0)
})()
